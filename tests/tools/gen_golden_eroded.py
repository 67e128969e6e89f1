"""Writes the fixtures of the IP-ERODED-3 / -11 tests (two-class INST heads, PostProcInstErodedMap) by running the REFERENCE on the CPU.
Needs /root/reference (read-only); never runs on the GPU machine.  Data only is stored.

    /opt/conda/bin/python3.9 tests/tools/gen_golden_eroded.py pp      -> tests/golden/pp_eroded.npz
        (the interpreter with the real scipy / scikit-image; OpenCV is absent: cv2 is oracle/cv2_standin.py, so the 11 x 11 ellipse follows
        OpenCV's documented span formula and is not pinned against OpenCV)
    python tests/tools/gen_golden_eroded.py net                       -> tests/golden/net_eroded_mixed96.npz, net_eroded_g448.npz
    python tests/tools/gen_golden_eroded.py train                     -> tests/golden/train_eroded.npz
        (the interpreter with torch)

pp:    every case stores the one-channel input and the label map of the reference's PostProcInstErodedMap.post_process; the test-side restatement
       (tests/eroded_ref.py) must equal it before anything is written.  The reference squeezes its input (np.squeeze, loader/postproc.py:154): on
       a map with a side of one pixel it raises before it labels anything -- those cases ("ref_raised") store the restatement's map.
net:   oracle.gen_golden_net.run_case, unmodified; afterwards the per-pixel logits and margins are dropped from the file (the tests compare logits
       with the oracle, which run_case has just held to the reference), which keeps each file below 1 MiB.
train: the reference's own train_step on the mixed model, built the way oracle/gen_golden_train_loss.py::run_case("paramset/") builds its case.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
GOLDEN = os.path.join(TESTS, "golden")

MIXED = [("Lumen", [("INST", 2)]), ("Gland", [("INST", 3)]), ("Nuclei", [("INST", 2)]), ("Nuclei#TYPE", [("TYPE", 7)]), ("Gland#TYPE", [("TYPE", 3)]),
         ("Patch-Class", [("OUT", 9)])]
ALL2 = [("Lumen", [("INST", 2)]), ("Gland", [("INST", 2)]), ("Nuclei", [("INST", 2)]), ("Nuclei#TYPE", [("TYPE", 7)]), ("Gland#TYPE", [("TYPE", 3)]),
        ("Patch-Class", [("OUT", 9)])]


# ---------------------------------------------------------------------------------------------------------------------------------
def pp_cases():
    from oracle import synth

    def inner(m):
        return np.ascontiguousarray(m[..., 0])

    def rects(h, w, boxes, dtype=np.float32):
        m = np.zeros((h, w), dtype)
        for y0, y1, x0, x1, cut in boxes:
            m[y0:y1, x0:x1] = 1.0
            if cut:  # one pixel less: a corner
                m[y0, x0] = 0.0
        return m

    c = []
    # ---- nuclei ---------------------------------------------------------------------------------------------------------------
    c.append(("nuc_generic", "Nuclei", inner(synth.nuclei_maps(256, 256, 110, 1500.0, noise=0.02))))
    c.append(("nuc_ragged", "Nuclei", inner(synth.nuclei_maps(97, 131, 118, 3500.0, noise=0.02))))
    c.append(("nuc_border", "Nuclei", inner(synth.nuclei_maps(160, 160, 114, 3000.0, border_bias=True))))
    c.append(("nuc_holes", "Nuclei", inner(synth.blob_maps(192, 192, 115, 40, 6.0, 14.0, holes=0.7, noise=0.02))))
    c.append(("nuc_all_fg", "Nuclei", np.ones((48, 48), np.float32)))
    c.append(("nuc_empty", "Nuclei", np.zeros((64, 80), np.float32)))
    # components of exactly 7 and 8 pixels (min_size 8 keeps the second), a 3 x 3 ring of 8 with a one-pixel hole, a diagonal pair that 4-connectivity splits
    m = rects(40, 48, [(4, 6, 4, 8, True), (4, 6, 20, 24, False), (20, 24, 30, 32, True), (30, 34, 8, 10, False)])
    m[12:15, 36:39] = 1.0
    m[13, 37] = 0.0
    m[30:32, 30:34] = 1.0  # 8 px ...
    m[32:34, 34:38] = 1.0  # ... and 8 px touching it by a corner only: two components
    c.append(("nuc_7_and_8", "Nuclei", m))
    # ---- gland ----------------------------------------------------------------------------------------------------------------
    c.append(("gland_generic", "Gland", inner(synth.blob_maps(448, 448, 120, 16, 22.0, 48.0, noise=0.02, rim=4.0, sharp=1.0))))
    c.append(("gland_border", "Gland", inner(synth.blob_maps(384, 384, 122, 14, 20.0, 45.0, border_bias=True, rim=4.0, sharp=1.0))))
    c.append(("gland_holes", "Gland", inner(synth.blob_maps(400, 400, 123, 9, 30.0, 60.0, holes=1.0, rim=4.0, sharp=1.0))))
    c.append(("gland_touching", "Gland", inner(synth.blob_maps(416, 352, 127, 30, 20.0, 34.0, noise=0.03, rim=4.0, sharp=1.0))))
    c.append(("gland_empty", "Gland", np.zeros((96, 96), np.float32)))
    # the pad rule (2 * ksize = 22): a blob of 58 x 58 = 3364 px whose box is 21 px from every edge (no side is padded: the dilation is cut at the box),
    # 22 px (top / left are padded, bottom / right are not: x2 + 22 <= W - 1 fails by one) and 23 px (all four)
    for d in (21, 22, 23):
        m = rects(58 + 2 * d, 58 + 2 * d, [(d, d + 58, d, d + 58, False)])
        m[d + 20:d + 30, d + 20:d + 30] = 0.0  # a hole to fill
        m[d, d] = m[d + 57, d + 57] = 0.0      # and corners for the ellipse to round
        c.append(("gland_pad%d" % d, "Gland", m))
    c.append(("gland_1499_1500", "Gland", rects(120, 160, [(30, 60, 30, 80, True), (70, 100, 90, 140, False)])))
    # ---- lumen ----------------------------------------------------------------------------------------------------------------
    c.append(("lumen_generic", "Lumen", inner(synth.blob_maps(320, 320, 121, 14, 8.0, 30.0, noise=0.02, rim=3.0))))
    c.append(("lumen_small", "Lumen", inner(synth.blob_maps(200, 200, 126, 30, 3.0, 9.0, rim=1.0))))
    c.append(("lumen_149_150", "Lumen", rects(64, 72, [(10, 20, 10, 25, True), (30, 40, 40, 55, False)])))
    # ---- degenerate maps ------------------------------------------------------------------------------------------------------
    c.append(("deg_1x1", "Nuclei", np.ones((1, 1), np.float32)))
    m = np.ones((1, 37), np.float32)
    m[0, 20] = 0.0  # runs of 20 and 16 pixels
    c.append(("deg_1x37", "Nuclei", m))
    m = np.ones((5, 3), np.float32)
    m[2, 1] = 0.0
    c.append(("deg_5x3", "Nuclei", m))
    return c


def gen_pp():
    import oracle.cv2_standin as cv2_standin

    sys.modules["cv2"] = cv2_standin
    from loader.postproc import PostProcInstErodedMap as RefPP  # (reference)

    import eroded_ref

    store, names = {}, []
    for name, tissue, m in pp_cases():
        f32 = False  # (every input is stored as fp16: the file stays below 1 MiB; the threshold test reads the same values)
        m = np.ascontiguousarray(m, np.float32)
        if not f32:  # inputs exactly representable in fp16: a smaller fixture
            m = m.astype(np.float16).astype(np.float32)
        raw = m[..., None].copy()
        raised = False
        try:
            ref, typ = RefPP.post_process(raw, {"%s-INST" % tissue: [0, 1]}, tissue)
            assert typ is None
        except (IndexError, ValueError) as e:  # np.squeeze took a one-pixel side away: the reference has no answer for this map
            assert 1 in m.shape, (name, e)
            raised, ref = True, None
        mine = eroded_ref.proc(m, tissue)
        if ref is not None:
            assert ref.dtype == np.float64 and mine.dtype == ref.dtype and np.array_equal(mine, ref), (name, int((mine != ref).sum()))
            # the type map comes back unsqueezed
            r2, t2 = RefPP.post_process(np.concatenate([raw, raw], -1), {"%s-INST" % tissue: [0, 1], "%s-TYPE" % tissue: [1, 2]}, tissue, 0.5)
            assert t2.shape == m.shape + (1,) and np.array_equal(r2, ref)
        else:
            ref = mine
        print("%-16s %-6s %-10s n_inst=%4d fg=%.3f %s" % (name, tissue, m.shape, int(ref.max()), float((ref > 0).mean()),
                                                      "reference raised: restatement stored" if raised else "restatement == reference"))
        names.append(name)
        store["in/" + name] = m if f32 else m.astype(np.float16)
        store["out/" + name] = ref.astype(np.int32)
        store["tissue/" + name] = tissue
        store["ref_raised/" + name] = np.bool_(raised)
    store["names"] = np.array(names)
    path = os.path.join(GOLDEN, "pp_eroded.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


# ---------------------------------------------------------------------------------------------------------------------------------
def gen_net():
    from oracle import gen_golden_net as G
    from cerberus_amd.weights import default_model_kwargs

    tasks = list(default_model_kwargs()["considered_tasks"])
    for tag, kw in (("eroded_mixed96", dict(tile_seed=31, n=2, hw=96, out_shape=96, tasks=tasks, decoder_kwargs=MIXED)),
                    ("eroded_g448", dict(tile_seed=32, n=1, hw=448, out_shape=144, tasks=tasks, decoder_kwargs=ALL2))):
        G.run_case(tag, **kw)
        path = os.path.join(GOLDEN, "net_%s.npz" % tag)
        g = np.load(path)
        keep = {k: g[k] for k in g.files if not k.startswith(("logits_full/", "logits_crops/", "margin/"))}
        for k in keep:
            if k.startswith("out_full/") and k.endswith("INST"):
                print(tag, k, keep[k].shape)
        np.savez_compressed(path, **keep)
        print("slimmed", path, os.path.getsize(path) // 1024, "KiB")


# ---------------------------------------------------------------------------------------------------------------------------------
FULL = ["output_head.Nuclei.INST.x.1.conv.weight", "output_head.Nuclei.INST.x.1.conv.bias", "output_head.Nuclei.INST.x.0.block.0.conv.weight"]
LOGITS_STORED = ("Lumen-INST", "Gland-INST", "Nuclei-INST", "Gland-TYPE", "Patch-Class")  # Nuclei-TYPE: weight 0 in paramset.yml, its gradient is zero whatever the logits


def train_case(store):
    from collections import OrderedDict

    import torch
    import yaml
    from oracle import gen_golden_train_loss as T  # (the inert import stubs and the .to("cuda") shim; its reference imports)
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    torch.manual_seed(0)
    torch.set_num_threads(8)
    rs = np.random.RandomState(11)
    kw = default_model_kwargs()
    kw["decoder_kwargs"] = OrderedDict((k, OrderedDict(v)) for k, v in MIXED)
    model = T.create_model(**kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(0, kw["decoder_kwargs"], kw["considered_tasks"]).items()}, strict=True)
    net = torch.nn.DataParallel(model)
    opt = torch.optim.Adam(net.parameters(), lr=1.0e-3, betas=(0.9, 0.999))
    loss_kwargs = yaml.full_load(open("/root/reference/models/paramset.yml"))["loss_kwargs"]
    N, H = 3, 64
    heads = OrderedDict([("Lumen-INST", 2), ("Gland-INST", 3), ("Nuclei-INST", 2), ("Nuclei-TYPE", 7), ("Gland-TYPE", 3), ("Patch-Class", 9)])
    batch = {"img": torch.from_numpy(rs.randint(0, 256, (N, H, H, 3)).astype(np.uint8))}
    targets = {}
    for h, c in heads.items():
        if h == "Patch-Class":
            t = rs.randint(0, c, (N, 1, 1, 1))
        else:
            t = (rs.rand(N, H, H, 1) < 0.35) * rs.randint(1, c, (N, H, H, 1))
            t[:, :8] = 0
        targets[h] = t.astype(np.float32)
        batch[h] = torch.from_numpy(targets[h])
    has = np.full((N, len(heads)), None, dtype=object)
    for j, h in enumerate(heads):
        for n in range(N):
            if (n == 1 and h.startswith("Gland")) or (n == 2 and h == "Nuclei-TYPE"):
                continue
            has[n, j] = h
    batch["dummy_target"] = has
    captured, drop = {}, {}

    def hook(name):
        def f(mod, inp, out):
            out.retain_grad()
            captured[name] = out
        return f

    for dec, hd in model.output_head.items():
        for clf, mod in hd.items():
            mod.register_forward_hook(hook(dec.split("#")[0] + "-" + clf))
    model.decoder_head["Patch-Class"].register_forward_hook(hook("Patch-Class"))

    def drop_hook(mod, inp, out):
        drop["mask"] = (out != 0).detach().numpy() | (inp[0] == 0).detach().numpy()

    model.decoder_head["Patch-Class"].dropout.register_forward_hook(drop_hook)
    res = T.train_step(dict(batch), ({"net": {"desc": net, "optimizer": opt, "extra_info": {"loss": loss_kwargs}}}, None))
    import json

    store.update({"N": N, "H": H, "img": batch["img"].numpy(), "weight_seed": 0, "heads": np.array(list(heads.keys())), "n_classes": np.array(list(heads.values())),
                  "has_target": np.array([[x is not None for x in row] for row in has]), "dropout_mask": drop["mask"],
                  "decoder_kwargs_json": json.dumps(MIXED), "overall_loss": np.float64(res["EMA"]["overall_loss"])})
    for h in heads:
        lg = captured[h]
        g = lg.grad.numpy() if lg.grad is not None else np.zeros_like(lg.detach().numpy())
        store["dlogits/" + h] = g  # NCHW, as the reference's forward returns its logits
        if h in LOGITS_STORED:
            store["logits/" + h] = lg.detach().numpy()
        assert np.array_equal(targets[h], targets[h].astype(np.uint8))
        store["target/" + h] = targets[h].astype(np.uint8)  # NHWC with one channel, class ids
        store["loss/" + h] = np.float64(res["EMA"]["%s_loss" % h])
        print("%-12s logits %-18s loss %.6f  |dlogits| max %.3e" % (h, tuple(lg.shape), store["loss/" + h], np.abs(g).max()))
    prm = dict(model.named_parameters())
    for k in FULL:
        store["grad_full/" + k] = prm[k].grad.detach().numpy().astype(np.float32)
    store["grad_full_names"] = np.array(FULL)


def gen_train():
    import torch

    # the noise yardstick of the element-wise gradient comparison: the reference's own step through torch's two CPU convolution back ends
    torch.backends.mkldnn.enabled = False
    alt = {}
    train_case(alt)
    torch.backends.mkldnn.enabled = True
    store = {}
    train_case(store)
    for k in FULL:
        a, b = store["grad_full/" + k].astype(np.float64), alt["grad_full/" + k].astype(np.float64)
        store["grad_full_noise/" + k] = np.float64(np.abs(a - b).max() / max(np.abs(a).max(), 1e-30))
        print("noise %-55s %.3e" % (k, store["grad_full_noise/" + k]))
    path = os.path.join(GOLDEN, "train_eroded.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    what = sys.argv[1:] or ["pp"]
    for w in what:
        {"pp": gen_pp, "net": gen_net, "train": gen_train}[w]()
