"""Generate tests/golden/tissue_mask.npz: the REFERENCE's own misc/utils.py::stain_entropy_otsu / morphology / get_tissue_mask (lines 195-244) on
synthetic thumbnails and hand-made masks -- inputs, the stain byte planes, the combined entropy map, the Otsu threshold and every mask.

    python tests/tools/gen_golden_tissue_mask.py [--out FILE]     (reference checkout: $CERBERUS_REFERENCE, default <repository>/../reference)

Needs the real scikit-image (0.18.x) and scipy; cv2 is oracle/cv2_standin.py and the modules misc/utils.py imports but this path never calls are inert
stubs, as in gen_golden_targets.py.  Only DATA is written.

Images (SEED, one RandomState per image):
  glass   every pixel one of three near-white colours, (236..240 per channel), drawn with probabilities 0.90 / 0.05 / 0.05: faint noise
  tissue  ellipses filled with colours drawn uniformly from a 24-colour palette of pinks and purples (80..230 per channel): texture
  shapes  131 x 197, 192 x 256, 200 x 333 (two or three ellipses, one cut by an image border) and 9 x 11 (left part tissue; smaller than two
          footprints: all but the three pixels (4, 4..6) have fewer than 49 neighbours)
Masks: see mask_cases().  A mask of fewer than 2000 pixels always ends FULL in the reference (remove_small_holes fills a background component
below 2000 pixels whether or not it touches the border), so "neither empty nor full" is asserted on the final mask of the three larger images and on
the thresholded mask of the 9 x 11 one.

Nothing is written unless (all checked against the reference alone):
  * every image keeps its entropy values more than 1e-9 away from its threshold and from each of the 255 inner histogram edges,
  * the best between-class variance beats the runner-up (the best split that divides the pixels differently) by more than 1e-9 relative,
  * the restated stain-byte table, entropy sum, histogram and Otsu arithmetic reproduce the reference's values bit for bit,
  * each of the six morphology stages changes a pixel in at least one mask case, the object / hole sizes after erosion are the ones named below, the
    diagonal bridge is 8- but not 4-connected at the stage that labels it, and eroding with the outside counted as set would change a final mask.
"""
import hashlib
import os
import sys
from unittest.mock import MagicMock

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("CERBERUS_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
SEED = 20261018


def _import_reference():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    from oracle import cv2_standin

    sys.modules["cv2"] = cv2_standin
    for m in ["pandas", "tqdm", "termcolor", "matplotlib", "matplotlib.pyplot"]:
        if m not in sys.modules:
            try:
                __import__(m)
            except Exception:
                sys.modules[m] = MagicMock()
    import warnings

    warnings.simplefilter("ignore", DeprecationWarning)  # scipy.ndimage.morphology: the reference's import path
    import skimage.color  # noqa: F401  (the reference calls skimage.color.rgb2hed after a bare `import skimage`)
    from misc import utils as ref_utils  # noqa: E402  (reference)

    return ref_utils


# ---- images ----------------------------------------------------------------------------------------------------------------------------
def make_image(seed, h, w, ellipses):
    rs = np.random.RandomState(seed)
    glass = np.array([[238, 238, 238], [236, 239, 237], [240, 237, 239]], np.uint8)
    img = glass[rs.choice(3, size=(h, w), p=[0.90, 0.05, 0.05])]
    palette = np.stack([rs.randint(150, 231, 24), rs.randint(80, 181, 24), rs.randint(120, 221, 24)], -1).astype(np.uint8)
    tex = palette[rs.randint(0, 24, (h, w))]
    yy, xx = np.mgrid[0:h, 0:w]
    for cy, cx, a, b in ellipses:
        inside = ((yy - cy) / float(a)) ** 2 + ((xx - cx) / float(b)) ** 2 <= 1.0
        img[inside] = tex[inside]
    return np.ascontiguousarray(img)


IMAGES = [
    ("img131x197", 1, 131, 197, [(60, 70, 38, 48), (120, 170, 30, 40)]),        # the second ellipse is cut by the bottom and right borders
    ("img192x256", 2, 192, 256, [(70, 80, 45, 55), (150, 200, 30, 38), (10, 230, 25, 40)]),
    ("img200x333", 3, 200, 333, [(100, 0, 60, 50), (90, 230, 50, 70)]),         # the first one is cut by the left border
    ("img9x11", 4, 9, 11, [(4, 0, 20, 6)]),
]


# ---- the arithmetic restated (what the product's host side does), proven against the reference below -------------------------------------
def stain_table():
    from skimage.color import hed_from_rgb

    v = np.arange(256, dtype=np.float64)
    L = np.log(np.maximum(v / 255.0, 1e-6)) / np.log(1e-6)
    return L[None, :, None] * np.asarray(hed_from_rgb, np.float64)[:, None, :]  # [channel][value][stain]


def stain_bytes(img, lut):
    x = ((lut[0][img[..., 0]] + lut[1][img[..., 1]]) + lut[2][img[..., 2]]) * 255.0
    return (np.trunc(x).astype(np.int64) & 255).astype(np.uint8)


def otsu(counts, lo, hi):
    edges = np.linspace(lo, hi, 257)
    cen = (edges[:-1] + edges[1:]) / 2.0
    cnt = counts.astype(float)
    w1 = np.cumsum(cnt)
    w2 = np.cumsum(cnt[::-1])[::-1]
    m1 = np.cumsum(cnt * cen) / w1
    m2 = (np.cumsum((cnt * cen)[::-1]) / w2[::-1])[::-1]
    var = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return cen[int(np.argmax(var))], var, edges


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
def _dilated_area(bg):
    from scipy.ndimage import binary_dilation
    from skimage.morphology import disk

    return int(binary_dilation(np.pad(bg, 8), disk(3)).sum())


def _hole_with_dilated_area(target):
    """An a x b rectangle (a < 46, b < 60, first match) plus part of one more row whose dilation by disk(3) -- the hole as remove_small_holes sees it after the
    erosion -- has `target` pixels."""
    for a in range(30, 46):
        for b in range(30, 60):
            if not (42 * b - 300 <= target - (a - 36) * (b + 6) <= 42 * b + 400):  # (far from the target: skip the dilations)
                continue
            for extra in range(0, b):
                bg = np.zeros((a + 1, b), bool)
                bg[:a] = True
                bg[a, :extra] = True
                if _dilated_area(bg) == target:
                    return bg
    raise SystemExit("no hole shape with a dilated area of %d" % target)


def mask_cases():
    cases = []
    # objects: 46 x 56 rectangles erode to 40 x 50 = 2000 pixels; a missing pixel under the first eroded column costs one, four more pixels in a 47th row add one
    m = np.zeros((200, 300), bool)
    m[20:66, 20:76] = True
    m[65, 23] = False                       # -> 1999 after erosion
    m[20:66, 100:156] = True                # -> 2000
    m[20:66, 180:236] = True
    m[66, 180:184] = True                   # -> 2001
    m[90:93, 10:200] = True                 # structures thinner than the disk: 3 pixels, 1 pixel, a 6 x 6 block
    m[100, 10:250] = True
    m[110:116, 30:36] = True
    m[0:60, 250:300] = True                 # objects touching the top and right borders, ...
    m[120:200, 0:70] = True                 # ... the left and bottom ones
    m[150:200, 120:180] = True              # ... the bottom one only
    m[60:140, 292:300] = True               # eight columns on the right border below the block: scipy's erosion counts the outside as CLEAR and removes them
    cases.append(("objects", m))
    # holes in a mask that is set everywhere else (so it touches all four borders and both corners' rules)
    m = np.ones((330, 360), bool)
    y = 12
    for target, x in ((1999, 12), (2000, 80), (2001, 150)):
        bg = _hole_with_dilated_area(target)
        m[y:y + bg.shape[0], x:x + bg.shape[1]][bg] = False
    m[20:100, 250:330] = False              # 80 x 80: still above 2000 after the dilation, only binary_fill_holes closes it
    # two holes joined by a diagonal only once eroded: two one-pixel spikes, one pointing down and one pointing up, whose ends dilate to disks with tips at
    # (oy, ox + 1) and (oy + 1, ox) -- corner to corner
    oy, ox = 200, 200
    m[oy - 43:oy - 8, ox - 14:ox + 16] = False  # 35 x 30 block above ...
    m[oy - 8:oy - 2, ox + 1] = False            # ... with a spike down to (oy - 3, ox + 1)
    m[oy + 10:oy + 45, ox - 15:ox + 15] = False  # 35 x 30 block below ...
    m[oy + 4:oy + 10, ox] = False               # ... with a spike up to (oy + 4, ox)
    m[300:304, 40:300] = False              # a slit thinner than the disk
    cases.append(("holes", m))
    cases.append(("all_zero", np.zeros((64, 80), bool)))
    cases.append(("all_one", np.ones((64, 80), bool)))
    cases.append(("small_zero", np.zeros((30, 40), bool)))  # fewer than 2000 pixels: the background itself is a "small hole"
    rs = np.random.RandomState(SEED + 99)
    cases.append(("noise", rs.rand(150, 210) < 0.985))      # many small holes; the erosion leaves a sponge and a few small objects
    return cases


def morphology_stages(mask, border_value=0):
    """The reference's chain (misc/utils.py:216-235) stage by stage.  Its binary_erosion / binary_dilation are scipy's (misc/utils.py:16-19), whose
    border_value defaults to 0: the outside of the image counts as clear for BOTH (scikit-image's binary_erosion would count it as set)."""
    from scipy import ndimage
    from scipy.ndimage import binary_dilation, binary_erosion
    from skimage.morphology import disk, remove_small_holes, remove_small_objects

    s = [mask]
    s.append(binary_erosion(s[-1], disk(3), border_value=border_value))
    s.append(remove_small_holes(s[-1], area_threshold=2000, connectivity=1))
    s.append(remove_small_objects(s[-1], min_size=2000, connectivity=1))
    s.append(binary_dilation(s[-1], disk(3)))
    s.append(remove_small_holes(s[-1], area_threshold=2000, connectivity=1))
    s.append(ndimage.binary_fill_holes(s[-1]))
    return s


def main():
    out = os.path.join(ROOT, "tests", "golden", "tissue_mask.npz")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    ref = _import_reference()
    import warnings

    import skimage
    from scipy import ndimage
    from skimage.filters import rank, threshold_otsu
    from skimage.morphology import disk

    warnings.simplefilter("ignore", UserWarning)  # remove_small_objects: "only one label was provided"
    store = {"seed": np.int64(SEED)}
    lut = stain_table()
    names = []
    for nm, k, h, w, ell in IMAGES:
        img = make_image(SEED + k, h, w, ell)
        hed = (skimage.color.rgb2hed(img.copy()) * 255).astype(np.uint8)
        assert np.array_equal(stain_bytes(img, lut), hed), nm
        ents = [rank.entropy(hed[..., c], disk(4)) for c in range(3)]
        ent = np.sum([ents[0], ents[1]], axis=0) - ents[2]
        assert ent.dtype == np.float64 and np.array_equal(ent, (ents[0] + ents[1]) - ents[2]), nm
        thr = threshold_otsu(ent)
        lo, hi = float(ent.min()), float(ent.max())
        counts = np.histogram(ent.ravel(), bins=256, range=(lo, hi))[0]
        thr2, var, edges = otsu(counts, lo, hi)
        assert thr2 == thr, (nm, thr, thr2)
        # runner-up: the best split that divides the pixels differently (across an empty bin the same split repeats with bit-identical variance, and
        # argmax takes the first of them -- integer counts make that tie exact on every machine)
        w1 = np.cumsum(counts)[:-1]
        best = int(np.argmax(var))
        others = var[w1 != w1[best]]
        assert others.size and (var[best] - others.max()) > 1e-9 * var[best], (nm, var[best], others.max())
        assert np.abs(ent - thr).min() > 1e-9, nm
        inner = edges[1:-1]
        pos = np.clip(np.searchsorted(inner, ent.ravel()), 1, len(inner) - 1)
        assert np.minimum(np.abs(ent.ravel() - inner[pos - 1]), np.abs(ent.ravel() - inner[pos])).min() > 1e-9, nm
        m1 = ref.stain_entropy_otsu(img)
        assert np.array_equal(m1, ent > thr), nm
        m2 = ref.get_tissue_mask(img)
        assert m2.dtype == np.uint8 and np.array_equal(m2, ref.morphology(m1).astype(np.uint8)), nm
        probe = m2 if h * w >= 2000 else m1
        assert 0 < int(probe.sum()) < probe.size, (nm, int(probe.sum()))
        names.append(nm)
        store[nm + "/img"] = img
        store[nm + "/hed"] = hed
        store[nm + "/entropy"] = ent
        store[nm + "/threshold"] = np.float64(thr)
        store[nm + "/counts"] = counts.astype(np.int64)
        store[nm + "/stain_entropy_otsu"] = m1
        store[nm + "/get_tissue_mask"] = m2
        print(nm, img.shape, "threshold %.6f" % thr, "otsu mask %d px, tissue mask %d px" % (m1.sum(), m2.sum()), flush=True)
    store["images"] = np.array(names)

    changed = [False] * 6
    mnames = []
    four, eight = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    for nm, m in mask_cases():
        st = morphology_stages(m)
        got = ref.morphology(m)
        assert got.dtype == bool and np.array_equal(got, st[-1]), nm
        for i in range(6):
            changed[i] = changed[i] or not np.array_equal(st[i], st[i + 1])
        if nm == "objects":
            lab, n = ndimage.label(st[1], four)
            sizes = set(np.bincount(lab.ravel())[1:].tolist())
            assert {1999, 2000, 2001} <= sizes, sorted(sizes)
            assert not np.array_equal(morphology_stages(m, border_value=1)[-1], st[-1])  # the erosion's border rule reaches the result
            assert not st[1][88:118, :260].any()  # the thin structures are gone
        if nm == "holes":
            lab4, _ = ndimage.label(~st[1], four)
            sizes = np.bincount(lab4.ravel())
            assert {1999, 2000, 2001} <= set(sizes[1:].tolist()), sorted(sizes[1:].tolist())
            a, b = lab4[200, 201], lab4[201, 200]  # the two tips
            lab8, _ = ndimage.label(~st[1], eight)
            assert a > 0 and b > 0 and a != b and lab8[200, 201] == lab8[201, 200], "diagonal bridge"
            assert sizes[a] < 2000 and sizes[b] < 2000 and sizes[a] + sizes[b] >= 2000, (sizes[a], sizes[b])
            assert st[1][200, 200] and st[1][201, 201]
            assert not st[5][30:90, 260:320].any() and st[6][30:90, 260:320].all()  # the large hole: closed by binary_fill_holes alone
        mnames.append(nm)
        store["mask/" + nm + "/in"] = m
        store["mask/" + nm + "/out"] = got
        print("mask", nm, m.shape, int(m.sum()), "->", int(got.sum()), flush=True)
    assert all(changed), changed
    store["masks"] = np.array(mnames)

    # every colour there is: pixel i of a 4096 x 4096 image has colour (i >> 16, (i >> 8) & 255, i & 255)
    i = np.arange(1 << 24, dtype=np.uint32)
    allc = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    hed = (skimage.color.rgb2hed(allc) * 255).astype(np.uint8)
    assert np.array_equal(stain_bytes(allc, lut), hed)
    store["all_colours/sha256"] = np.array(hashlib.sha256(hed.tobytes()).hexdigest())
    pick = np.random.RandomState(SEED + 7).randint(0, 1 << 24, 4096)
    store["all_colours/sample_rgb"] = allc.reshape(-1, 3)[pick]
    store["all_colours/sample_hed"] = hed.reshape(-1, 3)[pick]
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
