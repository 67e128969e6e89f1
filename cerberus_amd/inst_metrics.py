"""Instance metrics on the device: panoptic quality (PQ = DQ x SQ, per class too), AJI, Dice2 and Dice1 between two int32 label maps.

    table = pair_table(true, pred)                  # PairTable: ids, areas and the sparse (true id, pred id, pixels) table, all on the device
    panoptic_quality(table), aji(table), dice2(table), dice1(table)
    panoptic_quality(table, type_true, type_pred, cls=k)      # multi-class PQ: the instances of class k only
    stats = InstanceStats(n_classes=0); stats.update(true, pred); stats.counters(); stats.scalars(); stats.reset()
    tile_instance_stats(model, img, ann_inst, ann_type=None, stats=None)   # infer_tiles -> post-processing -> update, no label map on the host
    remap_label(lab, by_size=False)                 # the reference's misc/utils.py:133-164

The definitions are written out in include/cerberus_hip.h (cerb_inst_*) and computed by csrc/inst_metrics.hip: an area pass per map, a pair pass
(LDS table per pixel tile, flushed into a global open-addressing table), a compaction, torch.sort on the K pairs, and a reduction.  Every decision
(match, arg-max, tie) is integer arithmetic; sum_iou is float64 added in one fixed order, so two runs agree bitwise.  The ratios are host float64.
There is no CPU path.

Ids need not be contiguous.  0 is background, and so is any id that is negative or above the stated bound (`max_true_id` / `max_pred_id`, by default
each map's own maximum).  Synchronisation: pair_table waits for the device once to read {n_pairs, overflow, n_true, n_pred} (the sizes of what it
returns), plus once before that for the two maxima when the bounds are not given, and once more per overflow retry.  Type vectors given by id are
checked against the largest id that occurs (one 4-byte read each); summary_device itself waits for nothing."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

SUMMARY = ("tp", "fp", "fn", "aji_inter", "aji_union", "dice2_inter", "dice2_total", "dice1_inter", "dice1_total", "n_true", "n_pred")
_WORDS = 12      # CERB_INST_SUMMARY_WORDS
_MAX_RETRIES = 12


def _need_gpu():
    if not torch.cuda.is_available():
        raise _lib.CerberusHipError("cerberus_amd needs a ROCm GPU; there is no CPU fallback")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _label_map(v, name, dev=None):
    """numpy array or tensor -> CUDA int32 [H, W] with unit column stride (a CUDA int32 tensor stays where it is, row-strided views included)."""
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    if not torch.is_tensor(v):
        raise TypeError("%s: label maps are numpy arrays or tensors, got %s" % (name, type(v).__name__))
    if v.dim() != 2:
        raise ValueError("%s: a label map is [H, W], got shape %s" % (name, tuple(v.shape)))
    if v.is_floating_point() or v.dtype == torch.bool:
        raise TypeError("%s: label maps hold integers, got %s" % (name, v.dtype))
    if dev is None:
        dev = v.device if v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if not v.is_cuda or v.device != dev:
        v = v.to(dev)
    if v.dtype != torch.int32:
        v = v.to(torch.int32)
    if v.numel() and v.stride(1) != 1:
        v = v.contiguous()
    return v


def _areas(lab, n_ids):
    """int64 [n_ids + 1]: pixels per id in [1, n_ids]."""
    area = torch.zeros(n_ids + 1, dtype=torch.int64, device=lab.device)
    h, w = int(lab.shape[0]), int(lab.shape[1])
    if n_ids > 0 and h > 0 and w > 0:
        _lib.check(_lib.lib().cerb_inst_areas(lab.data_ptr(), lab.stride(0), h, w, n_ids, area.data_ptr(), _stream(lab.device)))
    return area


def _ranks(area):
    """(index int32 [n_ids + 1]: 1-based rank of every id with area > 0 among them, 0 elsewhere; number of such ids as a 0-d tensor)"""
    present = area > 0
    incl = torch.cumsum(present.to(torch.int32), 0, dtype=torch.int32)
    return (incl * present).to(torch.int32), incl[-1]


def _compact(index, values, n):
    """values of the ids that occur, in ascending id order: [n] (n known on the host); ids that do not occur all land in a slot that is cut off."""
    buf = torch.zeros(int(index.numel()) + 1, dtype=values.dtype, device=values.device)
    buf.scatter_(0, index.to(torch.int64), values)
    return buf[1:n + 1].contiguous()


class PairTable(object):
    """The contingency table of two label maps on the device.  true_ids / pred_ids: int32, ascending, the ids that occur; true_area / pred_area: int64
    pixels of each; pairs: int64 [K, 3] rows (true id, pred id, pixels in both), sorted by (true id, pred id).  retries: how often the pair pass was
    repeated on a larger table; atomics: {'lds', 'global'} table updates of the last pass."""

    def __init__(self, true_ids, true_area, pred_ids, pred_area, keys, counts, shape, retries, atomics):
        self.true_ids, self.true_area, self.pred_ids, self.pred_area = true_ids, true_area, pred_ids, pred_area
        self._keys, self._counts = keys, counts  # (true rank << 32 | pred rank), sorted; pixels
        self.shape, self.retries, self.atomics = shape, retries, atomics
        self._pairs = None

    @property
    def device(self):
        return self.true_area.device

    @property
    def n_pairs(self):
        return int(self._keys.numel())

    @property
    def pairs(self):
        if self._pairs is None:
            if self.n_pairs == 0:
                self._pairs = torch.zeros((0, 3), dtype=torch.int64, device=self.device)
            else:
                t = self.true_ids.to(torch.int64)[(self._keys >> 32) - 1]
                p = self.pred_ids.to(torch.int64)[(self._keys & 0xFFFFFFFF) - 1]
                self._pairs = torch.stack([t, p, self._counts], 1)
        return self._pairs


def _capacity_for(n, floor=1024):
    cap = floor
    while cap < n:
        cap *= 2
    return cap


def pair_table(true, pred, max_true_id=None, max_pred_id=None, _capacity=None):
    """The PairTable of two label maps of one shape (numpy arrays or tensors; CUDA int32 tensors are read in place, row-strided views too).
    max_true_id / max_pred_id: the stated id bounds -- larger ids count as background; None: each map's maximum (one more wait for the device).
    _capacity: first size of the global pair table (tests; rounded up to a power of two)."""
    _need_gpu()
    t = _label_map(true, "true")
    p = _label_map(pred, "pred", t.device)
    if tuple(t.shape) != tuple(p.shape):
        raise ValueError("pair_table: the maps differ in shape: %s and %s" % (tuple(t.shape), tuple(p.shape)))
    dev = t.device
    h, w = int(t.shape[0]), int(t.shape[1])
    L = _lib.lib()
    with torch.cuda.device(dev):
        if h == 0 or w == 0:
            max_true_id = max_pred_id = 0
        elif max_true_id is None or max_pred_id is None:
            mx = torch.stack([t.max(), p.max()]).clamp_(min=0).cpu()
            max_true_id = int(mx[0]) if max_true_id is None else max_true_id
            max_pred_id = int(mx[1]) if max_pred_id is None else max_pred_id
        nt_ids, np_ids = int(max_true_id), int(max_pred_id)
        if nt_ids < 0 or np_ids < 0 or nt_ids >= 2 ** 31 - 1 or np_ids >= 2 ** 31 - 1:
            raise ValueError("pair_table: id bounds must lie in [0, 2^31 - 2]")
        area_t, area_p = _areas(t, nt_ids), _areas(p, np_ids)
        idx_t, n_t = _ranks(area_t)
        idx_p, n_p = _ranks(area_p)
        stream = _stream(dev)
        cap = _capacity_for(int(_capacity), 16) if _capacity is not None else _capacity_for(4 * min(nt_ids + np_ids, h * w // 16))
        # (first guess: four slots per possible instance, but no more than one per four pixels -- sparse ids would size it by their largest id;
        # a map with more pairs than that overflows once and is run again)
        retries = 0
        while True:
            if nt_ids == 0 or np_ids == 0:
                head, tab = torch.zeros(4, dtype=torch.int64, device=dev), None  # a side without labels: no pairs, no pass
            else:
                tab = torch.empty(int(L.cerb_inst_pairs_workspace_bytes(cap)) // 8, dtype=torch.int64, device=dev)
                _lib.check(L.cerb_inst_pairs(t.data_ptr(), t.stride(0), p.data_ptr(), p.stride(0), h, w, idx_t.data_ptr(), nt_ids, idx_p.data_ptr(), np_ids,
                                             tab.data_ptr(), cap, stream))
                head = tab[:4]
            # THE synchronisation: everything whose size the host must know travels in one copy
            k, overflow, a_lds, a_glob, nt, npr = [int(x) for x in torch.cat([head, torch.stack([n_t, n_p]).to(torch.int64)]).cpu()]
            if not overflow:
                break
            retries += 1
            if retries > _MAX_RETRIES:
                raise _lib.CerberusHipError("pair_table: the pair table still overflows at %d slots" % cap)
            cap *= 4
        if k > 0:
            keys = torch.empty(k, dtype=torch.int64, device=dev)
            counts = torch.empty(k, dtype=torch.int64, device=dev)
            n_out = torch.empty(1, dtype=torch.int64, device=dev)
            _lib.check(L.cerb_inst_pairs_compact(tab.data_ptr(), cap, keys.data_ptr(), counts.data_ptr(), k, n_out.data_ptr(), stream))
            keys, order = torch.sort(keys)
            counts = counts[order].contiguous()
        else:
            keys = torch.zeros(0, dtype=torch.int64, device=dev)
            counts = torch.zeros(0, dtype=torch.int64, device=dev)
        ids_t = torch.arange(nt_ids + 1, dtype=torch.int32, device=dev)
        ids_p = torch.arange(np_ids + 1, dtype=torch.int32, device=dev)
        return PairTable(_compact(idx_t, ids_t, nt), _compact(idx_t, area_t, nt), _compact(idx_p, ids_p, npr), _compact(idx_p, area_p, npr), keys, counts,
                         (h, w), retries, {"lds": a_lds, "global": a_glob})


def _type_vector(v, ids, name):
    """per-instance classes indexed by instance id -> int32 by rank, on the device"""
    if v is None:
        return None
    if isinstance(v, np.ndarray) or not torch.is_tensor(v):
        v = torch.as_tensor(np.asarray(v))
    if v.dim() != 1 or v.is_floating_point():
        raise ValueError("%s: a 1-D integer vector indexed by instance id" % name)
    v = v.to(ids.device)
    if ids.numel() and int(v.numel()) <= int(ids[-1]):  # (ids are ascending; one small read)
        raise ValueError("%s: %d entries do not cover instance id %d" % (name, int(v.numel()), int(ids[-1])))
    return v[ids.to(torch.int64)].to(torch.int32).contiguous()


def summary_device(table, type_true=None, type_pred=None, cls=None, match_iou=0.5, _by_rank=False):
    """The integer summary and sum_iou of a PairTable as device tensors (int64 [12] in the order of SUMMARY, float64 [1]); nothing waits.
    type_true / type_pred: classes indexed by instance id; cls: keep the instances of that class only."""
    if match_iou < 0.5:
        raise ValueError("panoptic_quality: match_iou below 0.5 needs an assignment solver (matches are unique only above 0.5); not built")
    if match_iou != 0.5:
        raise ValueError("panoptic_quality: only match_iou = 0.5 (IoU > 0.5) is built")
    if cls is not None and (type_true is None or type_pred is None):
        raise ValueError("panoptic_quality: cls needs type_true and type_pred")
    if cls is not None and int(cls) < 0:
        raise ValueError("panoptic_quality: cls must be >= 0")
    _need_gpu()
    dev = table.device
    tt = tp = None
    if cls is not None:
        tt = type_true if _by_rank else _type_vector(type_true, table.true_ids, "type_true")
        tp = type_pred if _by_rank else _type_vector(type_pred, table.pred_ids, "type_pred")
    L = _lib.lib()
    nt, npr, k = int(table.true_area.numel()), int(table.pred_area.numel()), table.n_pairs
    with torch.cuda.device(dev):
        summ = torch.empty(_WORDS, dtype=torch.int64, device=dev)
        siou = torch.empty(1, dtype=torch.float64, device=dev)
        nb = int(L.cerb_inst_pair_stats_workspace_bytes(nt, npr))
        ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        _lib.check(L.cerb_inst_pair_stats(ptr(table._keys), ptr(table._counts), k, ptr(table.true_area), nt, ptr(table.pred_area), npr,
                                          tt.data_ptr() if tt is not None else None, tp.data_ptr() if tp is not None else None,
                                          -1 if cls is None else int(cls), summ.data_ptr(), siou.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(dev)))
    return summ, siou


def ratios(s):
    """dq, sq, pq, aji, dice2, dice1 from a counter dict (host float64; nan where a denominator is 0, dq and sq 0)."""
    nan = float("nan")
    den = s["tp"] + s["fp"] / 2 + s["fn"] / 2
    dq = s["tp"] / den if den else 0.0
    sq = s["sum_iou"] / s["tp"] if s["tp"] else 0.0
    return OrderedDict((("dq", dq), ("sq", sq), ("pq", dq * sq),
                        ("aji", s["aji_inter"] / s["aji_union"] if s["aji_union"] else nan),
                        ("dice2", 2 * s["dice2_inter"] / s["dice2_total"] if s["dice2_total"] else nan),
                        ("dice1", 2 * s["dice1_inter"] / s["dice1_total"] if s["dice1_total"] else nan)))


def _as_dict(summ, siou):
    d = OrderedDict((k, int(v)) for k, v in zip(SUMMARY, summ))
    d["sum_iou"] = float(siou)
    return d


def summary(table, type_true=None, type_pred=None, cls=None):
    """Counters (Python ints), sum_iou and the ratios of a PairTable as one dict."""
    summ, siou = summary_device(table, type_true, type_pred, cls)
    d = _as_dict(summ.cpu().tolist(), siou.cpu().item())
    d.update(ratios(d))
    return d


def panoptic_quality(table, type_true=None, type_pred=None, cls=None, match_iou=0.5):
    """{'dq', 'sq', 'pq', 'tp', 'fp', 'fn', 'sum_iou'}; with cls the instances of that class only (type vectors indexed by instance id)."""
    summ, siou = summary_device(table, type_true, type_pred, cls, match_iou)
    d = _as_dict(summ.cpu().tolist(), siou.cpu().item())
    r = ratios(d)
    return OrderedDict((k, r[k] if k in r else d[k]) for k in ("dq", "sq", "pq", "tp", "fp", "fn", "sum_iou"))


def aji(table):
    return summary(table)["aji"]


def dice2(table):
    return summary(table)["dice2"]


def dice1(table):
    return summary(table)["dice1"]


def majority_types(inst_map, type_map, max_id=None):
    """Per-instance majority class from cerb_inst_table's type counts (classes 0 .. 7), with get_inst_info_dict's rule (loader/postproc.py:60-71): the
    most frequent class, the second one when that is 0 and another occurs; ties go to the smaller class.  Returns an int32 CUDA vector indexed by
    instance id (entry 0 and ids that do not occur: 0)."""
    from .postproc import inst_table_device

    inst_map = _label_map(inst_map, "inst_map")
    if isinstance(type_map, np.ndarray):
        type_map = torch.from_numpy(np.ascontiguousarray(type_map))
    type_map = type_map.to(inst_map.device).to(torch.uint8)
    if type_map.shape != inst_map.shape:
        raise ValueError("majority_types: the maps differ in shape")
    if max_id is None:
        max_id = int(inst_map.max().clamp(min=0).item()) if inst_map.numel() else 0
    out = torch.zeros(max_id + 1, dtype=torch.int32, device=inst_map.device)
    if max_id == 0:
        return out
    clean = torch.where((inst_map > 0) & (inst_map <= max_id), inst_map, torch.zeros_like(inst_map)).contiguous()
    counts = inst_table_device(clean, type_map.contiguous(), max_id)[:, 8:16]
    rank = counts * 8 + torch.arange(7, -1, -1, device=counts.device)  # unique maxima: the smaller class wins a tie
    best = rank.argmax(1)
    other = rank[:, 1:].argmax(1) + 1
    second = (best == 0) & (counts[:, 1:].sum(1) > 0)
    out[1:] = torch.where(second, other, best).to(torch.int32)
    return out


def remap_label(lab, by_size=False):
    """The reference's remap_label (misc/utils.py:133-164): contiguous ids 1 .. n in ascending order of the old ids; by_size: in descending area,
    equal areas in ascending old id.  int32; a numpy map comes back as numpy, a tensor as a CUDA tensor.  A map without labels comes back as int32
    zeros (the reference returns its input object)."""
    _need_gpu()
    host = isinstance(lab, np.ndarray)
    m = _label_map(lab, "lab")
    h, w = int(m.shape[0]), int(m.shape[1])
    out = torch.zeros((h, w), dtype=torch.int32, device=m.device)
    if h == 0 or w == 0:
        return out.cpu().numpy() if host else out
    if int(m.min().item()) < 0:
        raise ValueError("remap_label: negative ids")
    n_ids = int(m.max().item())
    if n_ids > 0:
        with torch.cuda.device(m.device):
            area = _areas(m, n_ids)
            if by_size:
                present = area > 0
                # descending area, equal areas by ascending id, in ONE int64 key (largest area x (largest id + 1) < 2^62); ids that do not occur go last
                key = torch.where(present, (area.max() - area) * (n_ids + 1) + torch.arange(n_ids + 1, device=m.device), torch.full_like(area, 2 ** 62))
                order = torch.argsort(key)
                table = torch.zeros(n_ids + 1, dtype=torch.int32, device=m.device)
                table[order] = torch.arange(1, n_ids + 2, dtype=torch.int32, device=m.device)
                table = table * present
            else:
                table, _ = _ranks(area)
            table = table.to(torch.int32).contiguous()
            _lib.check(_lib.lib().cerb_relabel(m.data_ptr(), m.stride(0), table.data_ptr(), n_ids + 1, h, w, out.data_ptr(), out.stride(0), _stream(m.device)))
    return out.cpu().numpy() if host else out


class InstanceStats(object):
    """Accumulator over images: integer counters plus sum_iou, overall ('all') and per class 1 .. n_classes - 1 when n_classes > 0.  Summaries stay
    on the device until counters() / scalars() read them in one copy."""

    def __init__(self, n_classes=0):
        _need_gpu()
        self.n_classes = int(n_classes)
        self.reset()

    def reset(self):
        self._rows = []  # per image: (int64 [G, 12], float64 [G]) device tensors, G = 1 + classes
        self.images = 0

    def groups(self):
        return ["all"] + list(range(1, self.n_classes))

    def update(self, true, pred, type_true=None, type_pred=None, table=None):
        """One image.  type_true / type_pred: classes indexed by instance id (needed when n_classes > 0).  table: the PairTable when the caller has it."""
        if self.n_classes > 0 and (type_true is None or type_pred is None):
            raise ValueError("InstanceStats: per-class figures need type_true and type_pred")
        if table is None:
            table = pair_table(true, pred)
        summ, siou = [], []
        tt = tp = None
        if self.n_classes > 0:
            tt = _type_vector(type_true, table.true_ids, "type_true")
            tp = _type_vector(type_pred, table.pred_ids, "type_pred")
        for g in self.groups():
            s, f = summary_device(table) if g == "all" else summary_device(table, tt, tp, g, _by_rank=True)
            summ.append(s)
            siou.append(f)
        self._rows.append((torch.stack(summ), torch.cat(siou)))
        self.images += 1
        return table

    def _host(self):
        if not self._rows:
            g = len(self.groups())
            return np.zeros((0, g, _WORDS), np.int64), np.zeros((0, g), np.float64)
        return torch.stack([r[0] for r in self._rows]).cpu().numpy(), torch.stack([r[1] for r in self._rows]).cpu().numpy()

    def per_image(self):
        """[{group: counters + sum_iou + ratios}] per image."""
        summ, siou = self._host()
        out = []
        for i in range(summ.shape[0]):
            row = OrderedDict()
            for j, g in enumerate(self.groups()):
                d = _as_dict(summ[i, j].tolist(), siou[i, j])
                d.update(ratios(d))
                row[g] = d
            out.append(row)
        return out

    def counters(self):
        """{group: summed integer counters + sum_iou}.  sum_iou is added over the images in update order (host float64)."""
        summ, siou = self._host()
        out = OrderedDict()
        for j, g in enumerate(self.groups()):
            tot = [int(v) for v in summ[:, j].sum(0)] if summ.shape[0] else [0] * _WORDS
            s = 0.0
            for v in siou[:, j]:
                s += float(v)
            out[g] = _as_dict(tot, s)
        return out

    def scalars(self):
        """'<group>-<figure>' pooled (from the summed counters) and '<group>-<figure>-mean' (mean over the images of the per-image figure, nan ones
        skipped; nan without any), figures dq sq pq aji dice2 dice1; 'mpq' / 'mpq-mean': mean of the per-class pq."""
        out = OrderedDict()
        per = self.per_image()
        for g, d in self.counters().items():
            name = "all" if g == "all" else "class%d" % g
            for k, v in ratios(d).items():
                out["%s-%s" % (name, k)] = v
                vals = [p[g][k] for p in per if not np.isnan(p[g][k])]
                out["%s-%s-mean" % (name, k)] = float(np.mean(vals)) if vals else float("nan")
        if self.n_classes > 1:
            out["mpq"] = float(np.mean([out["class%d-pq" % k] for k in range(1, self.n_classes)]))
            out["mpq-mean"] = float(np.mean([out["class%d-pq-mean" % k] for k in range(1, self.n_classes)]))
        return out


def label_maps_device(model, img, tissues=None):
    """infer_tiles + the per-tissue post-processing on the device: {tissue: [int32 CUDA (H, W) per tile]}, {tissue: uint8 CUDA [N, H, W] or None}.
    The post-processing is chosen per tissue from the head's channel count, as cerberus_amd.tile does from the target code: two channels ->
    postproc_device (IP-ERODED-CONTOUR-*), one -> postproc_eroded_device (IP-ERODED-*)."""
    from .postproc import mask_lumen_by_gland, postproc_device, postproc_eroded_device

    _need_gpu()
    img = torch.as_tensor(img)
    if img.dim() == 3:
        img = img[None]
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError("tile_instance_stats: img is uint8 [N, H, W, 3] (or one [H, W, 3] tile)")
    h, w = int(img.shape[1]), int(img.shape[2])
    pred = model.infer_tiles(img.cuda().contiguous(), [h, w], type_dtype=torch.uint8)
    inst, types = OrderedDict(), OrderedDict()
    for key, v in pred.items():
        if not key.endswith("-INST"):
            continue
        tissue = key[:-5]
        if tissues is not None and tissue not in tissues:
            continue
        nch = int(v.shape[3])
        if nch not in (1, 2):
            raise NotImplementedError("%s: %d probability channels; the post-processings on the device read one (IP-ERODED-*) or two (IP-ERODED-CONTOUR-*)" % (key, nch))
        inst[tissue] = [(postproc_device(v[n], tissue) if nch == 2 else postproc_eroded_device(v[n], tissue))[0] for n in range(int(v.shape[0]))]
        types[tissue] = pred.get(tissue + "-TYPE")
    if "Lumen" in inst and "Gland" in inst:
        for lu, gl in zip(inst["Lumen"], inst["Gland"]):
            mask_lumen_by_gland(lu, gl)
    return inst, types


def tile_instance_stats(model, img, ann_inst, ann_type=None, stats=None):
    """Instance metrics of a model on annotated tiles.  img: uint8 [N, H, W, 3]; ann_inst: {tissue: int32 [N, H, W] instance maps} (the tissues to
    score, e.g. 'Nuclei'); ann_type: optional {tissue: uint8 [N, H, W] class maps} -- with it, per-class figures from the majority class of every
    annotated and every predicted instance (the model's '<tissue>-TYPE' map); stats: {tissue: InstanceStats} to accumulate into.  Returns that dict.
    The forward, the label maps and the tables stay on the device; per tile the host reads the few sizes pair_table needs."""
    _need_gpu()
    if not isinstance(ann_inst, dict) or not ann_inst:
        raise ValueError("tile_instance_stats: ann_inst is a dict {tissue: instance maps}")
    inst, types = label_maps_device(model, img, tissues=list(ann_inst))
    stats = OrderedDict() if stats is None else stats
    for tissue, ann in ann_inst.items():
        if tissue not in inst:
            raise KeyError("tile_instance_stats: the model has no %s-INST head" % tissue)
        ann = torch.as_tensor(ann)
        if ann.dim() == 2:
            ann = ann[None]
        if len(inst[tissue]) != int(ann.shape[0]):
            raise ValueError("tile_instance_stats: %d tiles, %d %s annotation maps" % (len(inst[tissue]), int(ann.shape[0]), tissue))
        typed = ann_type is not None and ann_type.get(tissue) is not None
        if typed and types.get(tissue) is None:
            raise KeyError("tile_instance_stats: the model has no %s-TYPE head for the annotated classes" % tissue)
        if tissue not in stats:
            n_cls = 0
            if typed:
                n_cls = [och for name, hname, och, key in model._decoders if key == tissue + "-TYPE"][0]
            stats[tissue] = InstanceStats(n_cls)
        for n, lab in enumerate(inst[tissue]):
            t = _label_map(ann[n], "ann_inst", lab.device)
            if typed:
                at = torch.as_tensor(ann_type[tissue])
                at = at[None] if at.dim() == 2 else at
                stats[tissue].update(t, lab, majority_types(t, at[n]), majority_types(lab, types[tissue][n]))
            else:
                stats[tissue].update(t, lab)
    return stats
