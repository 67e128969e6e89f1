"""Bit-exact parity of the on-GPU post-processing (through the C ABI) with the golden label maps captured from the
reference (tests/golden/pp_cases.npz) and with the C oracle on larger seeded maps."""
import os

import numpy as np
import pytest

import torch

from cerberus_amd.postproc import PostProcInstErodedContourMap, mask_lumen_by_gland, postproc_device
from oracle import postproc_ref as pr
from oracle import synth

pytestmark = pytest.mark.gpu


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "pp_cases.npz"))
    for name in [str(n) for n in g["names"]]:
        yield name, str(g["tissue/" + name]), float(g["ds/" + name]), g["in/" + name].astype(np.float32), g["out/" + name], str(g["dtype/" + name])


def test_golden_label_maps_bit_exact(golden_dir):
    """All 21 label maps captured from the reference's own post_process (real scikit-image / scipy), no exceptions: the
    quantised / saturated cases (nuc_plateau_ties, nuc_ties8, nuc_saturated ...) go through the on-device replay of skimage's
    heap (n_ambiguous > 0 -> ws_exact_kernel)."""
    flagged = []
    for name, tissue, ds, m, ref, dt in _cases(golden_dir):
        raw = np.zeros(m.shape[:2] + (2,), np.float32)
        raw[:] = m
        inst, typ = PostProcInstErodedContourMap.post_process(raw, {tissue + "-INST": [0, 2]}, tissue, ds_factor=ds)
        amb = int(PostProcInstErodedContourMap.last_info["n_ambiguous"].item())
        assert typ is None
        assert str(inst.dtype) == dt, (name, inst.dtype, dt)
        nmis = int((inst.astype(np.int32) != ref).sum())
        assert nmis == 0, (name, nmis, amb)
        if amb:
            flagged.append(name)
    assert "nuc_saturated" in flagged and "nuc_plateau_ties" in flagged, flagged  # the replay really ran on the tie-heavy cases


def test_tie_rule_contract_without_replay(golden_dir):
    """exact_ties=False keeps the raster-order tie break: n_ambiguous == 0 must still imply the reference's map (the rule is a
    proof, not a heuristic), and the cases it flags are the only ones allowed to differ."""
    for name, tissue, ds, m, ref, dt in _cases(golden_dir):
        if tissue != "Nuclei":
            continue
        got, info = postproc_device(torch.from_numpy(np.ascontiguousarray(m.astype(np.float32))).cuda(), "Nuclei", exact_ties=False)
        if int(info["n_ambiguous"].item()) == 0:
            assert np.array_equal(got.cpu().numpy(), ref), name


@pytest.mark.parametrize("gain,noise,dens", [(8.0, 0.5, 1500.0), (20.0, 0.5, 3000.0), (20.0, 0.0, 600.0)])
def test_saturated_core_maps_2048_bit_exact(gain, noise, dens):
    """Maps shaped like a confident trained head's output: float32 softmax whose nucleus cores are EXACTLY 1.0f (2-13 % of all
    pixels tie at the top priority).  gain 8: the floods prove for (all but one of) the 5205 regions that no tie can reach the labels; gain 20
    (cores one pixel apart): some regions depend on skimage's heap order and the replay reproduces it."""
    m = synth.softmax_nuclei_maps(2048, 2048, 7, dens, gain=gain, logit_noise=noise)
    assert float((m[..., 0] == 1.0).mean()) > 0.015
    ref = pr.proc(m, "Nuclei")
    got, info = postproc_device(torch.from_numpy(m).cuda(), "Nuclei")
    amb = int(info["n_ambiguous"].item())
    assert np.array_equal(got.cpu().numpy(), ref), (gain, amb)
    if gain <= 8.0:
        assert amb <= 2, amb  # 1 of 5205 regions on this seed (a conservative flag: the fast floods' map is identical too)
    else:
        assert amb > 0, "expected the heap replay to be exercised"
        fast, _ = postproc_device(torch.from_numpy(m).cuda(), "Nuclei", exact_ties=False)
        assert 0 < int((fast.cpu().numpy() != ref).sum()) < 2000  # raster-order ties: a few pixels per flagged region


@pytest.mark.parametrize("hw,seed,density", [((512, 512), 31, 1500.0), ((777, 1033), 32, 3000.0), ((2048, 2048), 33, 800.0)])
def test_nuclei_vs_oracle_large(hw, seed, density):
    m = synth.nuclei_maps(hw[0], hw[1], seed, density, noise=0.02)
    got, info = postproc_device(torch.from_numpy(m).cuda(), "Nuclei")
    ref = pr.proc(m, "Nuclei")
    assert np.array_equal(got.cpu().numpy(), ref)
    assert int(info["n_inst"].item()) >= int(ref.max())


@pytest.mark.parametrize("tissue,ds", [("Gland", 1.0), ("Lumen", 1.0), ("Gland", 0.5), ("Lumen", 0.5)])
def test_gland_lumen_vs_oracle(tissue, ds):
    m = synth.blob_maps(900, 1100, 41, 40, 14.0, 60.0, rim=4.0, sharp=1.0, noise=0.02, holes=0.3, border_bias=True)
    got, info = postproc_device(torch.from_numpy(m).cuda(), tissue, ds)
    ref = pr.proc(m, tissue, ds).astype(np.int32)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert int(info["n_inst"].item()) == int(ref.max()) or ref.max() == 0


def test_strided_canvas_window_and_lumen_mask():
    """Reads a window of a 9-channel canvas in place (no copy) -- the stitching layout of infer/tile.py:119-134."""
    H, W = 300, 420
    canvas = torch.zeros((H + 40, W + 60, 9), dtype=torch.float32, device="cuda")
    g = synth.blob_maps(H, W, 51, 14, 16.0, 44.0, rim=4.0, sharp=1.0)
    l = synth.blob_maps(H, W, 52, 20, 6.0, 16.0, rim=2.0)
    canvas[20:20 + H, 30:30 + W, 2:4] = torch.from_numpy(g).cuda()
    canvas[20:20 + H, 30:30 + W, 0:2] = torch.from_numpy(l).cuda()
    win = canvas[20:20 + H, 30:30 + W]
    gl, _ = postproc_device(win[..., 2:4], "Gland")
    lu, _ = postproc_device(win[..., 0:2], "Lumen")
    rg, rl = pr.proc(g, "Gland"), pr.proc(l, "Lumen")
    assert np.array_equal(gl.cpu().numpy(), rg.astype(np.int32))
    assert np.array_equal(lu.cpu().numpy(), rl.astype(np.int32))
    mask_lumen_by_gland(lu, gl)
    bg = rg.copy()
    bg[bg > 0] = 1
    assert np.array_equal(lu.cpu().numpy(), (bg * rl).astype(np.int32))  # infer/tile.py:187-191


def test_degenerate_maps():
    for m in [np.zeros((33, 47, 2), np.float32), np.ones((40, 40, 2), np.float32) * np.float32(0.3), np.ones((1, 1, 2), np.float32)]:
        for tissue in ("Nuclei", "Gland", "Lumen"):
            got, info = postproc_device(torch.from_numpy(np.ascontiguousarray(m)).cuda(), tissue)
            ref = pr.proc(m, tissue)
            assert np.array_equal(got.cpu().numpy(), ref.astype(np.int32)), (m.shape, tissue)


def test_idempotent_and_deterministic():
    m = torch.from_numpy(synth.nuclei_maps(640, 640, 61, 2500.0, noise=0.03)).cuda()
    a, _ = postproc_device(m, "Nuclei")
    b, _ = postproc_device(m, "Nuclei")
    assert torch.equal(a, b)


def test_instance_table_vs_oracle():
    """cerb_inst_table / get_inst_info_dict (box, centroid, majority type) vs the numpy restatement of loader/postproc.py:12-98 (itself
    pinned to the reference's function by tests/golden/inst_info.npz) on a larger map than the fixtures hold."""
    from cerberus_amd.postproc import get_inst_info_dict

    m = synth.blob_maps(700, 900, 71, 60, 10.0, 45.0, rim=4.0, sharp=1.0, noise=0.02, border_bias=True)
    lab, _ = postproc_device(torch.from_numpy(m).cuda(), "Gland")
    rs = np.random.RandomState(5)
    typ = (rs.rand(700, 900) < 0.6).astype(np.uint8) * rs.randint(1, 7, (700, 900)).astype(np.uint8)
    got = get_inst_info_dict(lab, torch.from_numpy(typ).cuda())
    ref = pr.inst_info_ref(lab.cpu().numpy(), typ)
    assert sorted(got.keys()) == sorted(ref.keys()) and len(got) > 5
    for k, d in got.items():
        r = ref[k]
        assert np.array_equal(d["box"], r["box"]) and np.allclose(d["centroid"], r["centroid"], rtol=0, atol=1e-9)
        assert d["contour"].dtype == np.int32 and np.array_equal(d["contour"], r["contour"]), k
        assert d["type"] == r["type"] and abs(d["type_prob"] - r["type_prob"]) < 1e-12
    half = get_inst_info_dict(lab, None, ds_factor=0.5)
    k0 = next(iter(got))
    assert np.array_equal(half[k0]["box"], np.round(got[k0]["box"] / 0.5).astype(int)) and "type" not in half[k0]
    assert np.array_equal(half[k0]["contour"], np.round(got[k0]["contour"] / 0.5).astype(int))
    assert get_inst_info_dict(torch.zeros((8, 8), dtype=torch.int32, device="cuda")) == {}


def test_instance_dictionary_vs_reference_fixture(golden_dir):
    """cerberus_amd.postproc.get_inst_info_dict (cerb_inst_table + cerb_inst_contour_* on the GPU) against the dictionaries the REFERENCE's
    own get_inst_info_dict returned for the golden label maps (tests/golden/inst_info.npz): key order, boxes, centroids, contours, the
    < 3-point skip, type votes incl. exact ties and background majorities, type_prob, ds_factor 1 and 0.5, with and without a type map."""
    from cerberus_amd.postproc import get_inst_info_dict
    from oracle import instinfo_fixture as fx

    n = 0
    for tag, lab, typ, ds, with_type, ref in fx.cases(golden_dir):
        got = get_inst_info_dict(torch.from_numpy(lab).cuda(), torch.from_numpy(typ).cuda() if with_type else None, ds_factor=ds)
        fx.check(got, ref, with_type, tag)
        n += 1
    assert n >= 20


def test_inst_table_first_pixel_and_relabel():
    """cerb_inst_table column 7 (first pixel in raster order) and cerb_relabel."""
    from cerberus_amd.postproc import inst_table_device
    from cerberus_amd.shard_postproc import _device_relabel_fn

    m = synth.nuclei_maps(512, 640, 21, 700.0, noise=0.02)
    lab, info = postproc_device(torch.from_numpy(m).cuda(), "Nuclei")
    n = int(info["n_inst"].item())
    tab = inst_table_device(lab, None, n).cpu().numpy()
    L = lab.cpu().numpy()
    ys, xs = np.nonzero(L)
    first = np.full(n, L.size, np.int64)
    np.minimum.at(first, L[ys, xs] - 1, ys * L.shape[1] + xs)
    assert np.array_equal(tab[:, 7], first)
    mapping = np.zeros(n + 1, np.int32)
    mapping[1:] = np.random.RandomState(1).permutation(n) + 100
    out = _device_relabel_fn(lab[100:300], torch.from_numpy(mapping).cuda()).cpu().numpy()
    assert np.array_equal(out, mapping[L[100:300]])


@pytest.mark.parametrize("tissue,ds", [("Nuclei", 1.0), ("Gland", 0.5), ("Lumen", 0.5)])
def test_sharded_postproc_equals_whole_map(tissue, ds):
    """SURVEY par.8e: three bands labelled locally (halo, ownership by first pixel, global id offsets) == the whole map labelled
    on one GPU, up to the id bijection; ids dense and ordered by (band, first pixel)."""
    from cerberus_amd import shard_postproc as sp

    H, W = 1536, 1024
    if tissue == "Nuclei":
        m = synth.nuclei_maps(H, W, 31, 600.0, noise=0.02)
    else:
        m = synth.blob_maps(H, W, 33, 60, 10.0, 40.0, rim=4.0, sharp=1.0, noise=0.02, holes=0.3)
    full = torch.from_numpy(m).cuda()
    ref, info = postproc_device(full, tissue, ds)
    n_ref = int(info["n_inst"].item())
    bands = [full[0:512], full[512:1024], full[1024:1536]]
    outs, n_total, infos = sp.run_local(bands, tissue, 192, 24, ds)
    assert all(i["n_truncated"] == 0 and i["n_unresolved"] == 0 for i in infos), infos
    lab = sp.assemble(outs).cpu().numpy()
    r = ref.cpu().numpy()
    n_alive = len(np.unique(r)) - 1  # glands overwritten entirely by a later paste leave no pixels
    assert n_total == n_alive and n_alive <= n_ref and n_alive > 20
    assert sorted(np.unique(lab)[1:]) == list(range(1, n_total + 1))
    assert sp.same_partition(r, lab)
    cross = (set(np.unique(lab[511])) & set(np.unique(lab[512]))) | (set(np.unique(lab[1023])) & set(np.unique(lab[1024])))
    assert len(cross - {0}) > 0
    # first pixels of the ids are increasing: (band, first pixel) order
    ys, xs = np.nonzero(lab)
    first = np.full(n_total, lab.size, np.int64)
    np.minimum.at(first, lab[ys, xs] - 1, ys * W + xs)
    assert np.all(np.diff(first) > 0)


def test_contours_nuclei_and_degenerate_shapes():
    """Border following (cerb_inst_contour_*) vs the Suzuki-Abe restatement on watershed nuclei (hundreds of small 4-connected
    regions), single pixels, one-pixel lines, diagonal chains (8-connected), a ring and an instance touching all four edges."""
    from cerberus_amd.postproc import get_inst_info_dict

    m = synth.nuclei_maps(600, 800, 9, 900.0, noise=0.05)
    lab, _ = postproc_device(torch.from_numpy(m).cuda(), "Nuclei")
    got = get_inst_info_dict(lab)
    ref = pr.inst_info_ref(lab.cpu().numpy())
    assert sorted(got.keys()) == sorted(ref.keys()) and len(got) > 200
    for k in got:
        assert np.array_equal(got[k]["contour"], ref[k]["contour"]), k
    L = np.zeros((40, 48), np.int32)
    L[0:40, 0] = 1; L[0, 0:48] = 1; L[39, 0:48] = 1; L[0:40, 47] = 1   # frame touching every edge
    L[5, 5] = 2                                                          # single pixel -> dropped (< 3 points)
    L[8, 4:20] = 3                                                       # horizontal line -> 2 points -> dropped
    for i in range(8):
        L[12 + i, 6 + i] = 4                                             # diagonal chain (8-connected only)
    L[24:34, 10:22] = 5; L[27:31, 13:19] = 0                             # ring: outer border only
    L[10:20, 30:33] = 6; L[14, 33:40] = 6; L[12:17, 40] = 6              # T / comb shape
    got = get_inst_info_dict(L)
    ref = pr.inst_info_ref(L)
    assert sorted(got.keys()) == sorted(ref.keys()) == [1, 5, 6]
    for k in got:
        assert np.array_equal(got[k]["contour"], ref[k]["contour"]), k
    assert got[5]["contour"].tolist() == [[10, 24], [10, 33], [21, 33], [21, 24]]


def test_contour_of_an_instance_in_several_pieces():
    """A lumen cut by its gland's edge, or a gland partly overwritten by a later one, is several 8-connected pieces under one id.
    findContours(...)[0][0] (loader/postproc.py:29-33) is then the border of the piece found LAST in the raster scan (OpenCV lists
    top-level contours most-recently-found first): cerb_inst_contour_start picks that piece; pieces joined only diagonally are one."""
    from cerberus_amd.postproc import get_inst_info_dict

    L = np.zeros((60, 70), np.int32)
    L[2:12, 3:15] = 1       # piece A of instance 1 (first in raster order)
    L[20:33, 40:60] = 1     # piece B
    L[33:40, 60:66] = 1     # joined to B through one diagonal contact (32,59)-(33,60): same piece
    L[45:50, 5:30] = 1      # piece C: starts last -> its border is the one reported
    L[15:30, 5:20] = 2      # instance 2, one piece, with a hole
    L[20:25, 10:15] = 0
    L[52:58, 40:44] = 3     # instance 3: two pieces side by side on the same rows -> the right one starts later
    L[52:58, 50:57] = 3
    rs = np.random.RandomState(0)
    R = (rs.rand(90, 110) < 0.55).astype(np.int32) * rs.randint(1, 6, (90, 110))  # salt: ids in many 8-connected fragments
    for lab in (L, R):
        got = get_inst_info_dict(lab)
        ref = pr.inst_info_ref(lab)
        assert sorted(got.keys()) == sorted(ref.keys())
        for k in got:
            assert np.array_equal(got[k]["contour"], ref[k]["contour"]), k
    got = get_inst_info_dict(L)
    assert got[1]["contour"].tolist() == [[5, 45], [5, 49], [29, 49], [29, 45]]
    assert got[3]["contour"].tolist() == [[50, 52], [50, 57], [56, 57], [56, 52]]


def test_instance_dictionary_of_a_label_map_with_more_than_2_31_pixels():
    """A 0.5-mpp scan of a large section (60000 x 50000) is a label map past int32 pixel indices: cerb_inst_table, cerb_inst_contour_start (its
    union-find takes int64 labels there, 8 bytes of workspace per pixel) and the border following must give, for instances planted at the map's far
    end (every pixel index > 2^31), exactly the entries they give for the same instances on a small map -- shifted."""
    from cerberus_amd.postproc import get_inst_info_dict

    L = np.zeros((60, 70), np.int32)
    L[2:12, 3:15] = 1       # instance 1 in three pieces: the last one found is the one reported
    L[20:33, 40:60] = 1
    L[33:40, 60:66] = 1
    L[45:50, 5:30] = 1
    L[15:30, 5:20] = 2      # one piece with a hole
    L[20:25, 10:15] = 0
    L[52:58, 40:44] = 3     # two pieces on the same rows
    L[52:58, 50:57] = 3
    small = get_inst_info_dict(L)
    H, W = 32768 + 64, 65536
    assert H * W >= 2 ** 31
    big = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    y0, x0 = H - 60, W - 70
    assert y0 * W + x0 > 2 ** 31
    big[y0:, x0:] = torch.from_numpy(L).cuda()
    got = get_inst_info_dict(big)
    del big
    assert sorted(got.keys()) == sorted(small.keys()) == [1, 2, 3]
    for k in small:
        assert np.array_equal(got[k]["contour"], small[k]["contour"] + np.array([x0, y0])), k
        assert np.array_equal(np.asarray(got[k]["box"]).reshape(-1), np.asarray(small[k]["box"]).reshape(-1) + np.array([y0, x0, y0, x0])), k
        assert np.allclose(got[k]["centroid"], np.asarray(small[k]["centroid"]) + np.array([x0, y0]), atol=1e-6), k
    from cerberus_amd import postproc as pp

    pp._ws_cache.clear()  # (17 GB of union-find labels: not something the rest of the suite should keep)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("tissue", ["Nuclei", "Gland", "Lumen"])
def test_postproc_is_bitwise_reproducible(tissue):
    """The CCL / flood kernels use atomics and lock-free union-find; the label maps must not depend on scheduling."""
    m = synth.nuclei_maps(1024, 1280, 41, 800.0, noise=0.05) if tissue == "Nuclei" else \
        synth.blob_maps(1024, 1280, 43, 80, 10.0, 50.0, rim=4.0, sharp=1.0, noise=0.05, holes=0.4)
    md = torch.from_numpy(m).cuda()
    ref, info0 = postproc_device(md, tissue)
    for _ in range(4):
        lab, info = postproc_device(md, tissue)
        assert torch.equal(lab, ref) and int(info["n_inst"]) == int(info0["n_inst"])


def test_sharded_postproc_flags_instances_taller_than_the_margin():
    """The band result is only claimed exact when n_truncated == n_unresolved == 0: an instance that does not fit into the halo
    must be counted, never silently cut."""
    from cerberus_amd import shard_postproc as sp

    H, W = 1200, 400
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W, 2), np.float32)
    m[..., 0] = ((yy - 600) ** 2 + (xx - 200) ** 2 < 180 ** 2).astype(np.float32)   # one gland, 360 rows tall, centred on the band edge
    m[..., 0] += ((yy - 100) ** 2 + (xx - 100) ** 2 < 40 ** 2).astype(np.float32)    # and a small one well inside band 0
    full = torch.from_numpy(m).cuda()
    outs, n_total, infos = sp.run_local([full[:600], full[600:]], "Gland", 128, 16, 1.0)
    assert sum(i["n_truncated"] + i["n_unresolved"] for i in infos) >= 1, infos
    # with a margin that holds the instance the same map is exact again
    outs, n_total, infos = sp.run_local([full[:600], full[600:]], "Gland", 320, 16, 1.0)
    assert all(i["n_truncated"] == 0 and i["n_unresolved"] == 0 for i in infos), infos
    ref, _ = postproc_device(full, "Gland", 1.0)
    assert n_total == 2 and sp.same_partition(ref.cpu().numpy(), sp.assemble(outs).cpu().numpy())


def test_slide_scale_map_invariants_and_tiling_consistency():
    """A 8192 x 8192 structured map (57 k nuclei; too large for the oracle to finish in test time) through properties that do not
    depend on its size: ids are within 1..n (the markers' ids), every labelled pixel lies in the mask's support, and -- since
    the watershed is independent per mask component -- every component that lies wholly inside a 2048 x 2048 crop is partitioned
    exactly as when that crop is post-processed on its own (a checksum-of-tiles property: the crop result IS compared with the C
    oracle, the slide-scale result with the crop)."""
    from cerberus_amd.postproc import inst_table_device

    H = W = 8192
    m = synth.nuclei_maps(H, W, 7, 1000.0, noise=0.02)
    dev = torch.from_numpy(m).cuda()
    lab, info = postproc_device(dev, "Nuclei")
    n = int(info["n_inst"])
    assert n > 50000 and int(lab.max()) <= n and int(info["n_ambiguous"]) == 0
    tab = inst_table_device(lab, None, n).cpu().numpy()
    alive = tab[:, 0] > 0
    assert alive.mean() > 0.95  # markers with no mask pixel left (erosion) disappear; the rest keep their id
    assert int(lab.min()) == 0 and int(tab[alive, 0].sum()) == int((lab > 0).sum())  # every labelled pixel belongs to an id in 1..n
    assert int(((lab > 0) & ~(dev.sum(-1) > 0.5)).sum()) == 0  # labels only inside inner + contour > 0.5
    # tiling consistency on one crop: components fully inside the crop (not touching its edge ring) keep their partition
    y0, x0, S = 3000, 4100, 2048
    crop = np.ascontiguousarray(m[y0:y0 + S, x0:x0 + S])
    exp = pr.proc(crop, "Nuclei").astype(np.int32)  # the C oracle on the crop
    got_crop, _ = postproc_device(torch.from_numpy(crop).cuda(), "Nuclei")
    assert np.array_equal(got_crop.cpu().numpy(), exp)
    big = lab[y0:y0 + S, x0:x0 + S].cpu().numpy()
    from scipy import ndimage

    msk = (crop.sum(-1) > 0.5)
    comp, _ = ndimage.label(msk)  # a superset of the eroded mask's components: safe for the "touches the ring" test
    ring = np.zeros_like(msk)
    ring[:3], ring[-3:], ring[:, :3], ring[:, -3:] = True, True, True, True
    bad = np.unique(comp[ring & msk])
    inner = msk & ~np.isin(comp, bad)
    a, b = big[inner], exp[inner]
    assert inner.sum() > 100000 and np.array_equal(a > 0, b > 0)
    pairs = np.unique(np.stack([a[a > 0], b[a > 0]], axis=1), axis=0)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))  # a bijection between the two labellings


# ---- W2: the reference's tiled nuclei post-processing (infer/wsi.py:81-268, 642-684) on the GPU ------------------------------------------
@pytest.mark.parametrize("seed,dens,hw,tile,margin", [(5, 300.0, (700, 900), 256, 32), (6, 600.0, (640, 1000), 320, 32), (7, 150.0, (1100, 1300), 512, 64)])
def test_reference_tiling_on_device_equals_the_oracle_scheme(seed, dens, hw, tile, margin):
    """cerberus_amd/ref_tiling.py (`run_infer_wsi.py --reference_tiling`: the reference's four tile sets and margin rules, every tile labelled
    by cerb_postproc_nuclei, boxes from cerb_inst_table) against oracle/wsi_tiles_ref.py (the same scheme restated on the CPU with the C
    oracle as the labeller), scaled down so that a small map has many seams:
      (i)   the oracle's scheme run with the HIP kernel as its per-tile labeller keeps exactly the instances it keeps with the C oracle;
      (ii)  the product module returns exactly that instance set (boxes in slide coordinates), none twice;
      (iii) every one of them is an instance of the band scheme's result (sharded_postprocess == the whole-map labelling) with the identical
            box -- the reference's set is a subset; what it loses lies within one margin of an inner tile edge."""
    # (instances are identified by their boxes; get_inst_info_dict drops contours of fewer than 3 points like the reference does, which a
    # nucleus of >= 10 pixels -- remove_small_objects, loader/postproc.py:355 -- only has as a 1-pixel-wide line: none in these maps)
    from cerberus_amd import ref_tiling as rt
    from oracle import wsi_tiles_ref as wt

    m = synth.nuclei_maps(hw[0], hw[1], seed, dens, noise=0.02)
    dev = torch.from_numpy(m).cuda()

    def hip_labeller(crop):
        return postproc_device(torch.from_numpy(crop).cuda(), "Nuclei")[0].cpu().numpy()

    ref_c = wt.reference_tiled_nuclei(m, tile_shape=tile, margin=margin, patch_output_shape=16)
    ref_hip = wt.reference_tiled_nuclei(m, tile_shape=tile, margin=margin, patch_output_shape=16, labeller=hip_labeller)
    assert ref_hip == ref_c and len(ref_c) > 100                                                              # (i)
    got = rt.reference_tiled_nuclei(dev, None, tile_shape=tile, margin=margin, patch_output_shape=16)
    boxes = sorted(tuple(int(v) for v in d["box"]) for d in got.values())
    assert boxes == ref_c and len(set(boxes)) == len(boxes)                                                   # (ii)
    for d in list(got.values())[:50]:  # dictionaries are in slide coordinates: the centroid lies inside its box, the contour on / inside it
        x0, y0, x1, y1 = [int(v) for v in d["box"]]
        assert x0 <= d["centroid"][0] < x1 and y0 <= d["centroid"][1] < y1
        c = np.asarray(d["contour"])
        assert c[:, 0].min() >= x0 and c[:, 0].max() < x1 and c[:, 1].min() >= y0 and c[:, 1].max() < y1
    lab, _ = postproc_device(dev, "Nuclei", exact_ties=False)  # the whole-map labelling == the band scheme (test_sharded_postproc_equals_whole_map)
    whole = set(tuple(int(v) for v in b) for b in wt._inst_boxes(lab.cpu().numpy().astype(np.int64)).values())
    lost = whole - set(boxes)
    assert not (set(boxes) - whole) and len(lost) <= 0.05 * len(whole), (len(lost), len(whole))              # (iii)
    for x0, y0, x1, y1 in lost:
        near_x = min(abs(e - k * tile) for k in range(1, hw[1] // tile + 1) for e in (x0, x1))
        near_y = min(abs(e - k * tile) for k in range(1, hw[0] // tile + 1) for e in (y0, y1))
        assert min(near_x, near_y) <= margin, (x0, y0, x1, y1)


def test_reference_tiling_at_the_reference_geometry_loss_rate():
    """4096-pixel tiles, 64-pixel margins (infer/wsi.py:299-302) on a 9000 x 8600 structured map (a 3 x 3 tile grid with every strip / cross
    section kind): the reference's scheme on the GPU keeps a subset of the band scheme's instances with identical boxes and loses well
    under 1 % of them (printed: the number DESIGN.md quotes), all within one margin of an inner tile edge."""
    from cerberus_amd import ref_tiling as rt
    from cerberus_amd.postproc import inst_table_device

    H, W, tile, margin = 8600, 9000, 4096, 64
    eff = (tile // 144) * 144  # tiles hold whole output patches: 28 x 144 = 4032 pixels (infer/wsi.py:299-302 through _get_tile_info)
    t = torch.from_numpy(synth.nuclei_maps(2048, 2048, 31, 600.0, noise=0.02)).cuda()
    dev = t.repeat(-(-H // 2048), -(-W // 2048), 1)[:H, :W].contiguous()
    got = rt.reference_tiled_nuclei(dev, None, tile_shape=tile, margin=margin, patch_output_shape=144)
    boxes = [tuple(int(v) for v in d["box"]) for d in got.values()]
    assert len(set(boxes)) == len(boxes)
    lab, _ = postproc_device(dev, "Nuclei", exact_ties=False)  # == the band scheme's result
    tab = inst_table_device(lab).cpu().numpy()
    tab = tab[tab[:, 0] > 0]
    whole = set((int(r[5]), int(r[3]), int(r[6]), int(r[4])) for r in tab)  # cerb_inst_table: rows 3..6 = y1, y2, x1, x2 -> (x1, y1, x2, y2)
    lost = whole - set(boxes)
    assert not (set(boxes) - whole)
    rate = len(lost) / max(1, len(whole))
    print("reference tiling 4096 / 64 on %d x %d: %d of %d band-scheme instances lost (%.3f %%)" % (H, W, len(lost), len(whole), 100.0 * rate))
    assert len(whole) > 40000 and rate < 0.01
    for x0, y0, x1, y1 in lost:
        near_x = min(abs(e - k * eff) for k in (1, 2) for e in (x0, x1))
        near_y = min(abs(e - k * eff) for k in (1, 2) for e in (y0, y1))
        assert min(near_x, near_y) <= margin, (x0, y0, x1, y1)


def test_reference_tiling_two_tiles_wide_equals_the_oracle_instance_for_instance(golden_dir):
    """at the reference's own geometry (4096-pixel tiles, 64-pixel margins, 256-pixel output patches) on a slide two tiles
    wide and two tall (8192 x 8192: a 2 x 2 grid, one vertical and one horizontal strip pair, one cross section) the product path
    (cerberus_amd/ref_tiling.py, every tile labelled on the GPU with skimage's tie order) returns exactly the instances of the CPU oracle of
    the scheme (oracle/wsi_tiles_ref.py with the C oracle as labeller), box for box.  The oracle's answer for this seeded map is cached in
    tests/golden/ref_tiling_8192.npz (oracle/gen_golden_ref_tiling.py: running it here took 756 s of the GPU suite); the map is rebuilt from its
    seed and checked against the fixture's hash.  The live oracle still runs beside the product in the scaled-down cases above."""
    import hashlib

    from cerberus_amd import ref_tiling as rt

    g = np.load(os.path.join(golden_dir, "ref_tiling_8192.npz"))
    t = synth.nuclei_maps(2048, 2048, 17, 600.0, noise=0.02)
    m = np.tile(t, (4, 4, 1))
    assert m.shape == (8192, 8192, 2) and hashlib.sha1(m.tobytes()).hexdigest() == str(g["map_sha1"])
    prof = {}
    got = rt.reference_tiled_nuclei(torch.from_numpy(m).cuda(), None, tile_shape=4096, margin=64, patch_output_shape=256, prof=prof)
    boxes = sorted(tuple(int(v) for v in d["box"]) for d in got.values())
    ref = [tuple(int(v) for v in b) for b in g["boxes"]]
    assert prof["tiles_total"] == 4 + 2 + 2 + 1 and len(ref) > 30000
    assert boxes == ref and len(set(boxes)) == len(boxes)


_AB_SCRIPT = r"""
import hashlib, sys
import numpy as np, torch
from cerberus_amd.postproc import postproc_device
from cerberus_amd import synth_maps as synth
h = hashlib.sha1()
for (H, W, seed, dens) in [(512, 768, 3, 1500.0), (515, 773, 4, 3000.0), (1024, 1024, 5, 600.0)]:
    m = torch.from_numpy(synth.nuclei_maps(H, W, seed, dens, noise=0.05)).cuda()
    lab, info = postproc_device(m, "Nuclei")
    h.update(lab.cpu().numpy().tobytes())
    h.update(str(int(info["n_inst"])).encode())
print("LABELS", h.hexdigest())
"""


def _labels_digest(env_extra):
    import subprocess
    import sys

    env = dict(os.environ)
    env.pop("CERB_PP_ONE_PIXEL_THREADS", None)
    env.update(env_extra)
    env.pop("CERB_DEV_LIB", None)
    if env_extra:  # the switches exist only in the developers' build of the library (csrc/cerb_dev.h); the default run is the PRODUCT library's
        env["CERB_DEV_LIB"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _AB_SCRIPT], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return [l for l in out.stdout.splitlines() if l.startswith("LABELS")][-1]


def test_every_front_variant_gives_the_same_labels():
    """The nuclei front has two schedules: four pixels per thread, and the one-pixel-per-thread passes that a map whose width is not a multiple of four
    or whose label map is not 16-byte aligned takes.  CERB_PP_ONE_PIXEL_THREADS (developers' build; read once per process, so each variant runs in its own
    interpreter) sends every map through the one-pixel passes behind the four-pixel threshold and erosion -- the mixed schedule a misaligned label map
    gets.  It must label three seeded maps -- one with a width that is not a multiple of four, which takes the one-pixel passes throughout anyway -- to
    the same bytes as the product library's default."""
    want = _labels_digest({})
    for sw in ("CERB_PP_ONE_PIXEL_THREADS",):
        assert _labels_digest({sw: "1"}) == want, sw
