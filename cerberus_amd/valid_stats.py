"""Validation metrics on the device: the reference's ProcStepRawOutput callback (models/run_desc.py:606-747) and the scalar part of
proc_cum_epoch_step_output (:505-565).

    stats = ValidStats(channel_info)                       # one per validation run; holds the device accumulator
    stats.update(valid_step(batch, run_info)["raw"])       # the reference's protocol: the host arrays of valid_step
    stats.update_device(pred, true, dummy_target)          # CUDA tensors straight from NetDesc.infer_tiles / gen_targets_batch
    valid_step_stats(batch, run_info, stats)               # valid_step's forward + update_device: no head map crosses to the host
    validate(model, batches)                               # an epoch of valid_step_stats -> scalars()
    stats.counters(), stats.scalars(), stats.reset()

Per head and class the accumulator holds over_inter, over_total, over_correct and nr_pixels over the samples whose dummy_target row names the
head; the rules are written out in include/cerberus_hip.h (cerb_valid_stats_*) and computed by csrc/valid_stats.hip in one launch per step.  There
is no CPU path.  The counts are integers, so the device result is exact and bitwise reproducible; `scalars()` is host float64 arithmetic with the
reference's two formulas and gives the reference's numbers with `==`.

The Patch-Class case.  The reference's statistics are defined only when no sample of the batch carries a Patch-Class target: with one, its
valid_step sends the dense heads' 'true' maps through F.interpolate in NHWC order, they come back [N, H, H, W], and the callback raises on the
comparison with the [N, H, W] predictions.  Here the same per-head rules run on the natural [N, H, W] maps in both cases.  `update(raw)` recognises
those [N, H, H, W] arrays of `cerberus_amd.train.valid_step` and takes the original map back out of them: the interpolation repeats the map along
the LAST axis (true4[n, y, x, :] = map[n, y, x]), so the map is true4[..., 0] (square tiles only; a non-square tile resamples the columns).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

MAX_HEADS = 8     # CERB_VALID_MAX_HEADS: heads per native call
MAX_CLASSES = 16  # CERB_VALID_MAX_CLASSES
STATS = ("over_inter", "over_total", "over_correct", "nr_pixels")
_KIND = {"INST": 0, "TYPE": 1, "OUT": 2}


def heads_of(channel_info):
    """channel_info (the model's decoder_info_list / valid_step's 'channel_info': decoder -> {head: channels}) -> OrderedDict output key ->
    (kind, classes), in the order of the predictions: '<decoder without #suffix>-<head>', 'Patch-Class' for that branch."""
    out = OrderedDict()
    for name, heads in channel_info.items():
        for hname, och in heads.items():
            if hname not in _KIND or (hname == "OUT") != (name == "Patch-Class"):
                raise KeyError("ValidStats: cannot place head %r of decoder %r (known: INST, TYPE, and OUT of Patch-Class)" % (hname, name))
            key = name if name == "Patch-Class" else "%s-%s" % (name.split("#")[0], hname)
            och = int(och)
            if och > MAX_CLASSES or och < (1 if hname == "OUT" else 2):
                raise ValueError("ValidStats: head %r has %d channels (supported: up to %d)" % (key, och, MAX_CLASSES))
            out[key] = (_KIND[hname], och)
    return out


def summarize(counters):
    """The scalar part of proc_cum_epoch_step_output (models/run_desc.py:526-561) from the nested counter dict: '*-INST' heads give
    '<head>-<k>-accu' and '-dice' per class, '*-TYPE' heads and Patch-Class '<head>-<k>-dice' per class plus '-avg-accu' and '-avg-dice'.
    (The INST averages the reference prints come from a variable leaked out of the previous head's loop; they are not part of its result.)"""
    scalar = OrderedDict()
    for head, cum in counters.items():
        accu_list, dice_list = [], []
        for k, v in cum.items():
            accu = (v["over_correct"] + 1.0e-8) / (v["nr_pixels"] + 1.0e-8)
            dice = 2 * v["over_inter"] / (v["over_total"] + 1.0e-8)
            if "INST" in head:
                scalar["%s-%s-accu" % (head, k)] = accu
            else:
                accu_list.append(accu)
                dice_list.append(dice)
            scalar["%s-%s-dice" % (head, k)] = dice
        if "INST" not in head:
            scalar["%s-avg-accu" % head] = np.mean(accu_list)
            scalar["%s-avg-dice" % head] = np.mean(dice_list)
    return scalar


def _squeezed(shape):
    return [int(d) for d in shape if int(d) != 1]


class PreparedStep(object):
    """One step's native calls with everything they read already on the device (ValidStats.prepare).  launch() queues them on the current stream and
    may be repeated; the handle keeps the device tensors alive."""

    def __init__(self, stats, calls, keep):
        self._stats, self._calls, self._keep = stats, calls, keep

    def launch(self):
        self._stats._launch(self._calls)


class ValidStats(object):
    """The epoch accumulator of ProcStepRawOutput on the device.  channel_info: decoder -> {head: channels} (NetDesc.decoder_info_list restricted to
    the model's decoders, or the 'channel_info' valid_step returns); heads: optional subset / order of output keys to accumulate."""

    def __init__(self, channel_info, heads=None, device=None):
        if not torch.cuda.is_available():
            raise _lib.CerberusHipError("cerberus_amd needs a ROCm GPU; there is no CPU fallback")
        known = heads_of(channel_info)
        self.heads = OrderedDict((h, known[h]) for h in (known if heads is None else heads))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._acc = torch.zeros((len(self.heads), MAX_CLASSES, 4), dtype=torch.int64, device=self.device)
        self.steps = 0

    # ---- input forms -----------------------------------------------------------------------------------------------------------------------
    def _to_dev(self, v):
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(np.ascontiguousarray(v))
        if not torch.is_tensor(v):
            raise TypeError("ValidStats: arrays must be numpy arrays or tensors, got %s" % type(v).__name__)
        return v.to(self.device)

    def _tile(self, pred, n, hw):
        """(h, w) of the step from the first dense prediction (squeezed or natural shape), or from the Patch-Class map."""
        if hw is not None:
            return int(hw[0]), int(hw[1])
        for key, (kind, och) in self.heads.items():
            dims = _squeezed(pred[key].shape)
            if kind == 0 and och > 2:
                if not dims or dims[-1] != och - 1:
                    raise ValueError("ValidStats: %s prediction of shape %s does not end in %d channels" % (key, tuple(pred[key].shape), och - 1))
                dims = dims[:-1]
            if kind == 2 and int(np.prod(dims, dtype=np.int64)) == n:
                continue
            if n > 1:
                if not dims or dims[0] != n:
                    raise ValueError("ValidStats: %s prediction of shape %s does not start with the %d samples of dummy_target" % (key, tuple(pred[key].shape), n))
                dims = dims[1:]
            if len(dims) != 2:
                raise ValueError("ValidStats: cannot read the tile size from the %s prediction of shape %s; pass hw=(h, w)" % (key, tuple(pred[key].shape)))
            return dims[0], dims[1]
        raise ValueError("ValidStats: no prediction map gives the tile size; pass hw=(h, w)")

    def _plan(self, pred, true, dummy, hw=None):
        """The native calls of one step: [(head table, flags, accumulator rows, n, h, w)] and the device tensors they point into."""
        has = np.asarray(dummy)
        if has.ndim != 2:
            raise ValueError("ValidStats: dummy_target must be [N, B], got shape %s" % (tuple(has.shape),))
        n = int(has.shape[0])
        for key in self.heads:
            if key not in pred or key not in true:
                raise KeyError("ValidStats: the step carries no %s for head %r" % ("prediction" if key not in pred else "true map", key))
        h, w = self._tile(pred, n, hw)
        p = h * w
        flags = np.stack([np.any(has == key, axis=-1) for key in self.heads]).astype(np.uint8)  # run_desc.py:642, per head
        calls, keep, keys = [], [], list(self.heads)
        with torch.cuda.device(self.device):
            flags_dev = torch.from_numpy(flags).to(self.device)
            for i0 in range(0, len(keys), MAX_HEADS):
                part = keys[i0:i0 + MAX_HEADS]
                hs = _lib.ValidHeads()
                hs.n_heads = len(part)
                for i, key in enumerate(part):
                    kind, och = self.heads[key]
                    pv, tv = self._to_dev(pred[key]), self._to_dev(true[key])
                    pfmt = tfmt = 0
                    if kind == 0:
                        pv = pv.to(torch.float32)
                        want = n * p * (och - 1)
                    elif kind == 1:
                        if pv.dtype != torch.uint8:
                            pv = pv.to(torch.int64)
                            pfmt = 1
                        want = n * p
                    else:
                        pv = pv.to(torch.float32)
                        pfmt = 1 if (pv.numel() == n and p != 1) else 0
                        want = n if pfmt else n * p
                    if pv.numel() != want:
                        raise ValueError("ValidStats: %s prediction of shape %s does not hold %d x %d x %d pixels" % (key, tuple(pv.shape), n, h, w))
                    if tv.dtype not in (torch.int32, torch.float32):
                        tv = tv.to(torch.float32 if tv.is_floating_point() else torch.int32)
                    if tv.numel() == n * p * h and kind != 2 and h > 1:
                        # valid_step's [N, H, H, W] array of a batch with a Patch-Class target (models/run_desc.py:414-420): the map repeated along the last axis
                        if h != w:
                            raise ValueError("ValidStats: the [N, H, H, W] 'true' array of a non-square tile does not hold the original map")
                        tv = tv.reshape(n, h, h, w)[..., 0]
                    elif tv.numel() == n and kind == 2 and p != 1:
                        tfmt |= 2
                    elif tv.numel() != n * p:
                        raise ValueError("ValidStats: %s true map of shape %s does not hold %d x %d x %d pixels" % (key, tuple(tv.shape), n, h, w))
                    if tv.dtype == torch.float32:
                        tfmt |= 1
                    pv, tv = pv.contiguous(), tv.contiguous()
                    keep.extend((pv, tv))
                    hs.kind[i], hs.n_classes[i], hs.pred_fmt[i], hs.true_fmt[i] = kind, och, pfmt, tfmt
                    hs.pred[i], hs.true_map[i] = pv.data_ptr(), tv.data_ptr()
                calls.append((hs, flags_dev[i0:], self._acc[i0:], n, h, w))
        return calls, keep

    def _launch(self, calls):
        L = _lib.lib()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for hs, flags, acc, n, h, w in calls:
                _lib.check(L.cerb_valid_stats_accumulate(C.byref(hs), flags.data_ptr(), n, h, w, acc.data_ptr(), stream))

    def _accumulate(self, pred, true, dummy, hw=None):
        calls, keep = self._plan(pred, true, dummy, hw)  # every head is checked before the first launch: a refused step adds nothing
        self._launch(calls)
        # `keep` (uploads, dtype conversions, .contiguous() copies) is dropped here while the launch may still be in flight.  That is safe because these
        # tensors were allocated on the current stream, the one the launch is queued on: the caching allocator hands their memory out again only to work
        # queued behind it.  Tensors the CALLER made on another stream get no such protection: the caller orders the streams (as for any torch op).
        self.steps += 1

    def prepare(self, pred, true, dummy_target, hw=None):
        """The step of update() / update_device() split in two: uploads, conversions and the head tables now, PreparedStep.launch() later and as often as
        wanted (each launch accumulates the step once more).  For timing the launch and for callers that replay a step."""
        return PreparedStep(self, *self._plan(pred, true, dummy_target, hw))

    # ---- the public protocol -----------------------------------------------------------------------------------------------------------------
    def update(self, raw, hw=None):
        """One step of the callback on valid_step's 'raw' dict: {'pred': {head: array}, 'true': {head: array}, 'dummy': [N, B] object array of
        head names / None, ...}.  Arrays may be numpy (uploaded) or CUDA tensors, torch.squeeze'd as the reference returns them or in their natural
        shapes ('*-INST' [N, H, W, C-1] float32; '*-TYPE' [N, H, W] uint8 / int64; 'Patch-Class' [N, H, W] or one value per sample; 'true' [N, H, W]
        with an optional trailing 1, int32 or float32).  N comes from 'dummy', which also settles the squeezed N = 1 case the reference gets wrong
        (:638).  hw: the tile size, needed only when a side is 1."""
        self._accumulate(raw["pred"], raw["true"], raw["dummy"], hw)

    def update_device(self, pred, true, dummy_target, hw=None):
        """update() for maps that already live on the device: pred as NetDesc.infer_tiles returns it, true as gen_targets_batch returns it (CUDA
        tensors; anything else is a TypeError -- this entry never uploads a map), dummy_target the [N, B] object array."""
        for name, d in (("pred", pred), ("true", true)):
            for key in self.heads:
                if key in d and not (torch.is_tensor(d[key]) and d[key].is_cuda):
                    raise TypeError("ValidStats.update_device: %s[%r] is not a CUDA tensor (update() takes host arrays)" % (name, key))
        self._accumulate(pred, true, dummy_target, hw)

    def reset(self):
        """A fresh epoch: clears the accumulator (asynchronously, on the current stream)."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cerb_valid_stats_reset(self._acc.data_ptr(), len(self.heads), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self.steps = 0

    def counters_int(self):
        """The accumulator as it is: int64 numpy [heads][MAX_CLASSES][4] (over_inter, over_total, over_correct, nr_pixels).  The one device-to-host
        copy (it waits for the steps queued so far)."""
        return self._acc.cpu().numpy()

    def counters(self):
        """The reference's nested dict {head: {class: {'over_inter', 'over_total', 'over_correct', 'nr_pixels'}}} as float64 (classes 1 .. C-1,
        Patch-Class 0 .. C-1; run_desc.py:701-725)."""
        acc = self.counters_int()
        out = OrderedDict()
        for i, (key, (kind, och)) in enumerate(self.heads.items()):
            out[key] = OrderedDict((k, OrderedDict((s, np.float64(acc[i, k, j])) for j, s in enumerate(STATS))) for k in range(0 if kind == 2 else 1, och))
        return out

    def scalars(self):
        """track_dict['scalar'] of proc_cum_epoch_step_output for the epoch so far (host float64, the reference's formulas)."""
        return summarize(self.counters())


def _channel_info(model):
    info = OrderedDict()
    for name, hname, och, _ in model._decoders:
        info.setdefault(name, OrderedDict())[hname] = och
    return info


def valid_step_stats(batch_data, run_info, stats):
    """valid_step (cerberus_amd.train.valid_step, models/run_desc.py:332-436) with the callback fused in: the same eval-mode forward (through the
    inference twin of a model in training mode), the targets uploaded as they are ('<head>': [N, H, W, 1], Patch-Class [N, 1, 1, 1]; CUDA tensors
    stay where they are) and one statistics launch into `stats`.  Returns {'raw': {'dummy', 'channel_info'}}: no head map crosses to the host and the
    host never waits for the forward or the statistics to finish.  What it does wait for is its own uploads: targets given as host arrays and the
    step's flag bytes (heads x N) are pageable host-to-device copies, which return once the data is staged; targets that are CUDA tensors cost nothing."""
    from .train import _eval_twin

    run_info, _ = run_info
    model = run_info["net"]["desc"]
    batch = dict(batch_data)
    img = torch.as_tensor(batch.pop("img"))
    has = np.asarray(batch.pop("dummy_target"))
    dev = torch.device("cuda", torch.cuda.current_device())
    h, w = int(img.shape[1]), int(img.shape[2])
    tiles = img.to(dev).float().to(torch.uint8).contiguous()
    pred = _eval_twin(model).infer_tiles(tiles, [h, w], type_dtype=torch.uint8)  # the same decisions as valid_step's int64 maps in an eighth of the bytes
    true = {}
    for key in stats.heads:
        t = batch[key]
        true[key] = t if (torch.is_tensor(t) and t.is_cuda) else torch.as_tensor(t).to(dev)
    stats.update_device(pred, true, has, hw=(h, w))
    return {"raw": {"dummy": has, "channel_info": _channel_info(model)}}


def validate(model, batches, stats=None):
    """An epoch of valid_step_stats over `batches` (dicts of the reference's batch protocol) -> the epoch's scalars.  stats: an accumulator to
    reuse (it is reset first); by default a fresh one for the model's heads."""
    if stats is None:
        stats = ValidStats(_channel_info(model))
    else:
        stats.reset()
    run_info = ({"net": {"desc": model}}, None)
    for batch in batches:
        valid_step_stats(batch, run_info, stats)
    return stats.scalars()
