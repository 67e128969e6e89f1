"""Tissue-mask handling of the slide driver (reference infer/wsi.py:533-569, 688-835), device-resident.

  load_mask            cv2.imread + BGR2GRAY + `> 0` (infer/wsi.py:533-536), through PIL (OpenCV is not a dependency)
  select_patches       which output boxes hold tissue (infer/wsi.py:559-569 -> tiatoolbox filter_coordinates): host geometry on
                       the low-resolution mask, like the patch list itself
  TissueRegions        cerb_label_mask + cerb_inst_table on the GPU: the connected components of the mask and their bounding
                       boxes (infer/wsi.py:381-391, 724-725)
  pclass_tissue_map    cerb_pclass_tissue_map (infer/wsi.py:688-716)
  postprocess_regions  per tissue region: crop the gland / lumen probability canvases, keep the region's own mask pixels, x0.5
                       resize (one fused kernel, cerb_downsample2_inst_region), post-process at ds_factor 0.5, lumen inside
                       gland, instance dictionary shifted to slide coordinates (infer/wsi.py:730-835)

  stain_entropy_otsu,  the mask generator the reference's docstring promises for a slide without a mask file (infer/wsi.py:509; misc/utils.py:
  morphology,          195-244), which its command line never reaches: stain bytes, local entropy, histogram, threshold and the morphology chain
  get_tissue_mask      are HIP kernels (csrc/tissue_mask.hip, over the labeller of csrc/pp_label.hip), the two tables and Otsu's arithmetic on 256 counts are numpy

Without a mask the reference builds an all-ones mask at slide resolution -> one region = the whole slide; that case never
materialises a mask here (region_lab NULL).  There is no CPU fallback: every map stays in HBM."""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .postproc import _workspace, get_inst_info_dict, inst_table_device, mask_lumen_by_gland, postproc_device, postproc_eroded_device


def load_mask(path):
    """-> uint8 [mh, mw] of 0 / 1.  PIL's 'L' conversion uses the same ITU-R 601 luma as cv2.COLOR_BGR2GRAY; masks are black /
    white images, for which `> 0` cannot differ."""
    from PIL import Image

    m = np.array(Image.open(path).convert("RGB").convert("L"))
    return (m > 0).astype(np.uint8)


def select_patches(mask, out_boxes_yx, slide_hw):
    """mask: uint8 [mh, mw]; out_boxes_yx: int [P, 2, 2] ((y0, x0), (y1, x1)) output boxes at slide resolution.
    A patch runs when its output box, scaled to the mask with np.ceil, covers at least one mask pixel (tiatoolbox 1.3.1
    SemanticSegmentor.filter_coordinates; un-vendored, restated).  Summed-area table instead of one slice per patch."""
    mh, mw = mask.shape
    sat = np.zeros((mh + 1, mw + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(mask > 0, axis=0, dtype=np.int64), axis=1)
    b = np.asarray(out_boxes_yx, np.float64)
    sy, sx = mh / slide_hw[0], mw / slide_hw[1]
    y0 = np.clip(np.ceil(b[:, 0, 0] * sy).astype(np.int64), 0, mh)
    y1 = np.clip(np.ceil(b[:, 1, 0] * sy).astype(np.int64), 0, mh)
    x0 = np.clip(np.ceil(b[:, 0, 1] * sx).astype(np.int64), 0, mw)
    x1 = np.clip(np.ceil(b[:, 1, 1] * sx).astype(np.int64), 0, mw)
    y1, x1 = np.maximum(y1, y0), np.maximum(x1, x0)
    return (sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]) > 0


class TissueRegions(object):
    """Connected components of the slide mask on the GPU.  .lab: CUDA int32 [mh, mw]; .boxes: [[rmin, rmax, cmin, cmax], ...] in
    mask coordinates, region k has label k + 1.  An empty mask gives the reference's single whole-mask region (no pixel of
    which carries its label, infer/wsi.py:389-390,745: every probability is then multiplied by 0)."""

    def __init__(self, mask_dev):
        assert mask_dev.is_cuda and mask_dev.dtype == torch.uint8 and mask_dev.dim() == 2 and mask_dev.stride(1) == 1
        mh, mw = int(mask_dev.shape[0]), int(mask_dev.shape[1])
        dev = mask_dev.device
        self.mask = mask_dev
        self.lab = torch.empty((mh, mw), dtype=torch.int32, device=dev)
        n = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _workspace(dev, mh, mw)
        st = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cerb_label_mask(mask_dev.data_ptr(), mask_dev.stride(0), mh, mw, self.lab.data_ptr(), n.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), C.c_void_p(st)))
        self.n = int(n.item())
        if self.n > 0:
            tab = inst_table_device(self.lab, None, self.n).cpu().numpy()
            self.boxes = [[int(t[3]), int(t[4]), int(t[5]), int(t[6])] for t in tab]
        else:
            self.boxes = [[0, mh, 0, mw]]


def pclass_tissue_map(pclass, mask_dev=None):
    """pclass: CUDA float32 [H, W] class canvas (row stride free) -> CUDA float32 [cvRound(H/4), cvRound(W/4)]"""
    assert pclass.is_cuda and pclass.dtype == torch.float32 and pclass.dim() == 2 and pclass.stride(1) == 1
    h, w = int(pclass.shape[0]), int(pclass.shape[1])
    out = torch.empty((int(round(h * 0.25)), int(round(w * 0.25))), dtype=torch.float32, device=pclass.device)
    mp, ms, mh, mw = None, 0, 0, 0
    if mask_dev is not None:
        assert mask_dev.is_cuda and mask_dev.dtype == torch.uint8 and mask_dev.stride(1) == 1
        mp, ms, mh, mw = mask_dev.data_ptr(), mask_dev.stride(0), int(mask_dev.shape[0]), int(mask_dev.shape[1])
    st = torch.cuda.current_stream(pclass.device).cuda_stream
    with torch.cuda.device(pclass.device):
        _lib.check(_lib.lib().cerb_pclass_tissue_map(pclass.data_ptr(), pclass.stride(0), h, w, mp, ms, mh, mw, out.data_ptr(), C.c_void_p(st)))
    return out


def half_inst_region(inst, region_lab=None, region_id=0):
    """x0.5 cv2-bilinear resize of an INST window (H, W, >=2) after keeping one region's mask pixels.  region_lab: CUDA int32
    window of the mask's label map covering the same area (any resolution) or None.  A one-channel window (H, W, 1) -- the map of a two-class
    INST head -- gives (H/2, W/2, 1) through cerb_downsample2_map_region."""
    assert inst.is_cuda and inst.dtype == torch.float32 and inst.dim() == 3 and (inst.stride(2) == 1 or inst.shape[2] == 1)
    L = _lib.lib()
    h, w = int(inst.shape[0]), int(inst.shape[1])
    nch = 1 if int(inst.shape[2]) == 1 else 2
    out = torch.empty((L.cerb_half_size(h), L.cerb_half_size(w), nch), dtype=torch.float32, device=inst.device)
    lp, ls, mh, mw = None, 0, 0, 0
    if region_lab is not None:
        assert region_lab.is_cuda and region_lab.dtype == torch.int32 and region_lab.stride(1) == 1
        lp, ls, mh, mw = region_lab.data_ptr(), region_lab.stride(0), int(region_lab.shape[0]), int(region_lab.shape[1])
    st = torch.cuda.current_stream(inst.device).cuda_stream
    with torch.cuda.device(inst.device):
        if nch == 1:
            _lib.check(L.cerb_downsample2_map_region(inst.data_ptr(), inst.stride(0), inst.stride(1), h, w, 1, lp, ls, mh, mw, int(region_id), out.data_ptr(),
                                                     C.c_void_p(st)))
        else:
            _lib.check(L.cerb_downsample2_inst_region(inst.data_ptr(), inst.stride(0), inst.stride(1), h, w, lp, ls, mh, mw, int(region_id), out.data_ptr(),
                                                      C.c_void_p(st)))
    return out


def postprocess_regions(canv, slide_hw, regions=None, with_info=True):
    """Gland / lumen label maps and instance dictionaries, one tissue region at a time (infer/wsi.py:730-835).
    canv: head key -> CUDA canvas at slide resolution; regions: TissueRegions or None (no mask = the whole slide).
    -> list of {'topleft': [cmin, rmin], 'inst': {'Gland': int32 CUDA map at x0.5 of the region crop, 'Lumen': ...},
                'info': {'Gland': {id: {...}}, 'Lumen': {...}}}
    The dictionaries carry the reference's coordinates, including its box arithmetic: `inst_info["box"] += [cmin, rmin]` adds the
    x offset to the row pair and the y offset to the column pair (infer/wsi.py:739,813) -- kept, a drop-in must return the same."""
    H, W = int(slide_hw[0]), int(slide_hw[1])
    tissues = [t for t in ("Gland", "Lumen") if t + "-INST" in canv]
    out = []
    if regions is None:
        todo = [(None, 0, H, 0, W, None)]
    else:
        ratio = regions.lab.shape[0] / H
        todo = []
        for k, (r0, r1, c0, c1) in enumerate(regions.boxes):
            win = regions.lab[r0:r1, c0:c1]
            todo.append((k + 1, int(round(r0 / ratio)), int(round(r1 / ratio)), int(round(c0 / ratio)), int(round(c1 / ratio)), win))
    for rid, rmin, rmax, cmin, cmax, win in todo:
        inst, tmaps = OrderedDict(), {}
        for t in tissues:
            crop = canv[t + "-INST"][rmin:rmax, cmin:cmax]
            if crop.shape[0] < 1 or crop.shape[1] < 1:
                continue
            half = half_inst_region(crop, win, rid if rid is not None else 0)
            # one channel: PostProcInstErodedMap on the masked, halved crop -- full-resolution parameters, its `scale` is never read (infer/wsi.py:792-794)
            inst[t], _ = postproc_eroded_device(half, t) if half.shape[2] == 1 else postproc_device(half, t, 0.5)
            tm = canv.get(t + "-TYPE")
            if tm is not None and with_info:
                sub = tm[rmin:rmax, cmin:cmax][::2, ::2][: half.shape[0], : half.shape[1]].contiguous()
                if win is not None:  # class ids outside the region's own mask pixels are 0 (infer/wsi.py:776)
                    ys = torch.clamp((torch.arange(sub.shape[0], device=sub.device, dtype=torch.float64) * 2 * (1.0 / (crop.shape[0] / win.shape[0]))).floor().long(), max=win.shape[0] - 1)
                    xs = torch.clamp((torch.arange(sub.shape[1], device=sub.device, dtype=torch.float64) * 2 * (1.0 / (crop.shape[1] / win.shape[1]))).floor().long(), max=win.shape[1] - 1)
                    sub = sub * (win[ys][:, xs] == rid).to(sub.dtype)
                tmaps[t] = sub
        if "Lumen" in inst and "Gland" in inst:
            mask_lumen_by_gland(inst["Lumen"], inst["Gland"])
        rec = {"topleft": [cmin, rmin], "inst": inst, "info": OrderedDict()}
        if with_info:
            shift = np.array([cmin, rmin])
            for t, lab in inst.items():
                d = get_inst_info_dict(lab, tmaps.get(t), 0.5)
                for v in d.values():
                    b = v["box"] + shift
                    v["box"] = np.array([b[0][1], b[0][0], b[1][1], b[1][0]])
                    v["contour"] = v["contour"] + shift
                    v["centroid"] = v["centroid"] + shift
                rec["info"][t] = d
        out.append(rec)
    return out


# ---- get_tissue_mask (misc/utils.py:195-244) ----------------------------------------------------------------------------------
# skimage.color.hed_from_rgb = inv([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]) (Ruifrok & Johnston's stain vectors), as scikit-image
# 0.18 holds it: rows = R, G, B, columns = H, E, D
HED_FROM_RGB = ((1.8779827368521353, -1.0076786862855642, -0.5561158181996245),
                (-0.06590806222356335, 1.1347303724996625, -0.13552179862837113),
                (-0.601907363439289, -0.48041418849705786, 1.5735880719641924))
ENTROPY_LOG2 = 0.6931471805599453  # the constant rank.entropy divides by
MIN_TISSUE_AREA = 2000             # remove_small_holes / remove_small_objects (misc/utils.py:224-230); fixed in cerb_tissue_morphology


def stain_table():
    """float64 [3, 256, 3] = [channel][value][stain]: rgb2hed's log(max(v / 255, 1e-6)) / log(1e-6) times the stain matrix.  A pixel's stain s is
    ((t[0, r, s] + t[1, g, s]) + t[2, b, s]); the reference keeps (hed * 255).astype(uint8) of it (misc/utils.py:198-199)."""
    v = np.arange(256, dtype=np.float64)
    lg = np.log(np.maximum(v / 255.0, 1e-6)) / np.log(1e-6)
    return lg[None, :, None] * np.asarray(HED_FROM_RGB, np.float64)[:, None, :]


def stain_bytes_host(rgb, table=None):
    """The stain bytes of uint8 [..., 3] colours in numpy: the statement cerb_tissue_hed implements (truncate toward zero, wrap modulo 256)."""
    t = stain_table() if table is None else table
    rgb = np.asarray(rgb)
    x = ((t[0][rgb[..., 0]] + t[1][rgb[..., 1]]) + t[2][rgb[..., 2]]) * 255.0
    return (np.trunc(x).astype(np.int64) & 255).astype(np.uint8)


def entropy_term_table():
    """float64 [50, 50]: [pop][count] = p * log(p) / log(2) with p = count / pop, as rank.entropy evaluates it per bin (libm log); 0 where count is 0
    or above pop."""
    t = np.zeros((50, 50), np.float64)
    for pop in range(1, 50):
        for c in range(1, pop + 1):
            p = c / float(pop)
            t[pop, c] = p * math.log(p) / ENTROPY_LOG2
    return t


def otsu_threshold(counts, lo, hi):
    """skimage.filters.threshold_otsu(image) for a float image with minimum lo, maximum hi and np.histogram(image, 256, (lo, hi))[0] == counts."""
    edges = np.linspace(lo, hi, 257)
    cen = (edges[:-1] + edges[1:]) / 2.0
    cnt = np.asarray(counts).astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = np.cumsum(cnt)
        w2 = np.cumsum(cnt[::-1])[::-1]
        m1 = np.cumsum(cnt * cen) / w1
        m2 = (np.cumsum((cnt * cen)[::-1]) / w2[::-1])[::-1]
        var = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return float(cen[int(np.argmax(var))])


_tm_tables = {}


def _tissue_tables(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _tm_tables.get(key)
    if t is None:
        _tm_tables[key] = t = (torch.from_numpy(stain_table()).to(dev), torch.from_numpy(entropy_term_table()).to(dev))
    return t


def _tissue_ws(dev, h, w):
    return _workspace(dev, h, w, nbytes=int(_lib.lib().cerb_tissue_workspace_bytes(h, w)))


def stain_planes(img):
    """img: CUDA uint8 [H, W, 3] (row stride free) -> CUDA uint8 [3, H, W]: (rgb2hed(img) * 255).astype(uint8), H / E / D (misc/utils.py:198-202)"""
    if not (torch.is_tensor(img) and img.is_cuda):
        raise _lib.CerberusHipError("the tissue mask is computed on the GPU: img must be a CUDA tensor; there is no CPU fallback")
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.stride(2) == 1 and img.stride(1) == 3, "img: uint8 [H, W, 3], pixels packed"
    h, w = int(img.shape[0]), int(img.shape[1])
    dev = img.device
    lut, _ = _tissue_tables(dev)
    planes = torch.empty((3, h, w), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cerb_tissue_hed(img.data_ptr(), img.stride(0), h, w, lut.data_ptr(), planes.data_ptr(), C.c_void_p(st)))
    return planes


def stain_entropy(planes):
    """planes: CUDA uint8 [3, H, W] -> (CUDA float64 [H, W] = (entropy(H) + entropy(E)) - entropy(D) over disk(4), CUDA float64 [2] = its min, max)
    (misc/utils.py:203-208)"""
    assert planes.is_cuda and planes.dtype == torch.uint8 and planes.dim() == 3 and planes.shape[0] == 3 and planes.is_contiguous()
    h, w = int(planes.shape[1]), int(planes.shape[2])
    dev = planes.device
    _, term = _tissue_tables(dev)
    ent = torch.empty((h, w), dtype=torch.float64, device=dev)
    minmax = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _tissue_ws(dev, h, w)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cerb_tissue_entropy(planes.data_ptr(), h, w, term.data_ptr(), ent.data_ptr(), minmax.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(st)))
    return ent, minmax


def entropy_histogram(ent, lo, hi):
    """-> int64 numpy [256] = np.histogram(ent, bins=256, range=(lo, hi))[0], counted on the device"""
    assert ent.is_cuda and ent.dtype == torch.float64 and ent.dim() == 2 and ent.is_contiguous()
    dev = ent.device
    edges = torch.from_numpy(np.linspace(lo, hi, 257)).to(dev)
    counts = torch.empty(256, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cerb_tissue_histogram(ent.data_ptr(), int(ent.shape[0]), int(ent.shape[1]), edges.data_ptr(), counts.data_ptr(), C.c_void_p(st)))
    return counts.cpu().numpy()


def _stain_entropy_otsu_parts(img):
    planes = stain_planes(img)
    ent, minmax = stain_entropy(planes)
    lo, hi = (float(v) for v in minmax.cpu().numpy())  # 16 bytes of metadata: the histogram's range
    if not lo < hi:
        # (threshold_otsu hands such an image's one value back and the reference's `entropy > threshold` is empty: there is nothing to separate)
        raise ValueError("the thumbnail has a single entropy value (%r): no threshold separates tissue from glass" % lo)
    counts = entropy_histogram(ent, lo, hi)
    thr = otsu_threshold(counts, lo, hi)
    h, w = int(ent.shape[0]), int(ent.shape[1])
    mask = torch.empty((h, w), dtype=torch.uint8, device=img.device)
    st = torch.cuda.current_stream(img.device).cuda_stream
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().cerb_tissue_threshold(ent.data_ptr(), h, w, C.c_double(thr), mask.data_ptr(), C.c_void_p(st)))
    return mask, {"planes": planes, "entropy": ent, "threshold": thr, "counts": counts, "range": (lo, hi)}


def stain_entropy_otsu(img):
    """misc/utils.py:195-213.  img: CUDA uint8 [H, W, 3] -> CUDA bool [H, W].  ValueError for an image with a single entropy value."""
    return _stain_entropy_otsu_parts(img)[0].view(torch.bool)


def morphology(mask):
    """misc/utils.py:216-235.  mask: CUDA bool (or uint8) [H, W] -> CUDA bool [H, W]"""
    if not (torch.is_tensor(mask) and mask.is_cuda):
        raise _lib.CerberusHipError("the tissue mask is computed on the GPU: mask must be a CUDA tensor; there is no CPU fallback")
    assert mask.dtype in (torch.bool, torch.uint8) and mask.dim() == 2
    m = mask.contiguous().view(torch.uint8)
    h, w = int(m.shape[0]), int(m.shape[1])
    out = torch.empty((h, w), dtype=torch.uint8, device=m.device)
    ws = _tissue_ws(m.device, h, w)
    st = torch.cuda.current_stream(m.device).cuda_stream
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().cerb_tissue_morphology(m.data_ptr(), h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), C.c_void_p(st)))
    return out.view(torch.bool)


def get_tissue_mask(img, return_parts=False):
    """misc/utils.py:238-244.  img: CUDA uint8 [H, W, 3] -> CUDA uint8 [H, W] of 0 / 1; return_parts: also {'planes': uint8 [3, H, W], 'entropy':
    float64 [H, W], 'threshold': float, 'counts': int64 numpy [256], 'range': (min, max), 'otsu_mask': bool [H, W]}."""
    m1, parts = _stain_entropy_otsu_parts(img)
    mask = morphology(m1).view(torch.uint8)
    if return_parts:
        parts["otsu_mask"] = m1.view(torch.bool)
        return mask, parts
    return mask


def thumbnail(reader, proc_res, units, ds):
    """The slide at 1 / ds of the processing resolution through the reader's read_bounds (which picks the pyramid level): uint8 numpy [h, w, 3].
    Read in row strips of about 16 Mpx of source (read_bounds resamples on one global grid, so the strips do not show)."""
    s = reader._scale(proc_res, units) / float(ds)
    tw, th = (max(1, int(v)) for v in reader.slide_dimensions(s, "baseline"))
    rows = max(1, int(16e6 // max(1, tw * ds * ds)))
    out = np.empty((th, tw, 3), np.uint8)
    for y0 in range(0, th, rows):
        y1 = min(th, y0 + rows)
        out[y0:y1] = reader.read_bounds((0, y0, tw, y1), resolution=s, units="baseline")[..., :3]
    return out
