"""Training augmentations, host side (no GPU): the restatement tests/augs_ref.py against the published known answers of
tests/golden/augs_documented.json, and cerberus_amd.augs.sample_params / compose_map -- determinism, ranges, the frozen draw order
(tests/golden/augs_params_seed11.json) and the integer folding of crop and flips."""
import json
import os

import numpy as np
import pytest

import augs_ref as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def doc():
    return json.load(open(os.path.join(GOLDEN, "augs_documented.json")))


# ---- the restatement reproduces every known answer ----------------------------------------------------------------------------------------------------
def test_gaussian_tables(doc):
    for k in (1, 3, 5):
        e = doc["gaussian_kernel_sigma0"]["k%d" % k]
        assert R.GAUSS[k] == e["weights"] and sum(R.GAUSS[k]) == e["denominator"]
    # an impulse of 16 * 16 through the 5 x 5 blur returns the outer product of the table, exactly
    img = np.zeros((1, 9, 9, 3), np.uint8)
    img[0, 4, 4] = 255
    out = R.gaussian_blur(img, [5], [5])[0, 2:7, 2:7, 0].astype(np.int64)
    w = np.array(R.GAUSS[5])
    assert np.array_equal(out, (np.outer(w, w) * 255 + 128) >> 8)


def test_grey_of_primaries(doc):
    e = doc["grey_of_primaries"]
    assert R.grey(np.array(e["rgb"], np.uint8)).tolist() == e["grey"]


def test_hsv_of_documented_colours(doc):
    e = doc["hsv_8bit"]
    assert R.rgb_to_hsv(np.array(e["rgb"], np.uint8)).tolist() == e["hsv"]
    # and back: the documented colours survive the round trip
    assert R.hsv_to_rgb(np.array(e["hsv"])).tolist() == e["rgb"]


def test_philox_known_answer_two_restatements(doc):
    e = doc["philox4x32_10_zero"]
    want = [int(h, 16) for h in e["output_hex"]]
    assert R.philox_scalar(e["counter"], e["key"]) == want
    c = [np.array([v], np.uint64) for v in e["counter"]]
    assert [int(v[0]) for v in R.philox_vec(*c, e["key"][0], e["key"][1])] == want
    # the two restatements agree away from zero too
    rng = np.random.RandomState(3)
    cs = rng.randint(0, 2 ** 32, size=(16, 4), dtype=np.uint64)
    k0, k1 = 0x12345678, 0x9ABCDEF0
    vec = np.stack(R.philox_vec(cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3], k0, k1), 1)
    for i in range(16):
        assert R.philox_scalar([int(v) for v in cs[i]], [k0, k1]) == [int(v) for v in vec[i]]


def test_noise_exclusion_share_of_the_gpu_test_seeds():
    """The GPU test demands equality wherever the restatement's pre-floor value lies at least 1e-6 from an integer; the share of pixels it excludes is
    computed from the restatement alone and must stay below 0.1 % (expected about 2e-6) for the keys that test uses."""
    import augs_cases

    img, sigma, pc, key = augs_cases.noise_case()
    _, pre = R.gaussian_noise(img, sigma, pc, key)
    share = float(augs_cases.noise_excluded(pre).mean())
    print("excluded share %.3e" % share)
    assert share <= 1e-3


# ---- sample_params ------------------------------------------------------------------------------------------------------------------------------------
def _params(seed, n=8, src=(60, 52), out=(48, 40)):
    from cerberus_amd import augs

    return augs.sample_params(n, src, out, np.random.RandomState(seed))


def test_same_seed_same_parameters():
    a, b, c = _params(5), _params(5), _params(6)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    assert not np.array_equal(a["map"], c["map"])


def test_every_value_inside_its_documented_range():
    from cerberus_amd import augs

    P = augs.TRAIN_POLICY
    n, src, out = 400, (60, 52), (48, 40)
    p = augs.sample_params(n, src, out, np.random.RandomState(1))
    assert (p["scale"] >= 0.8).all() and (p["scale"] < 1.2).all() and P["scale"] == (0.8, 1.2)
    assert (np.abs(p["shear"]) <= 5.0).all() and (np.abs(p["rotate"]) <= 179.0).all()
    assert (np.abs(p["translate"][:, 0]) <= 0.01 * src[1]).all() and (np.abs(p["translate"][:, 1]) <= 0.01 * src[0]).all()
    assert 0.4 < p["fliplr"].mean() < 0.6 and 0.4 < p["flipud"].mean() < 0.6
    g, m, s = (p["gauss_k"] != 0).any(1), p["median_k"] != 0, np.isfinite(p["noise_sigma"])
    assert (g.astype(int) + m + s == 1).all() and g.any() and m.any() and s.any()  # exactly one of the three
    assert np.isin(p["gauss_k"][g], (1, 3, 5)).all() and np.isin(p["median_k"][m], (1, 3, 5)).all()
    assert set(np.unique(p["gauss_k"][g])) == {1, 3, 5} == set(np.unique(p["median_k"][m]))
    assert (p["noise_sigma"][s] >= 0).all() and (p["noise_sigma"][s] < 12.75).all()
    assert set(np.unique(p["noise_per_channel"][s])) == {0, 1} and len(np.unique(p["noise_key"][s])) == s.sum()
    assert (np.sort(p["colour_order"], 1) == np.arange(4)).all() and len(np.unique(p["colour_order"], axis=0)) > 12
    for name, bound in (("hue", 8.0), ("saturation", 0.2), ("brightness", 26.0)):
        assert (np.abs(p[name]) <= bound).all(), name
    assert (p["contrast"] >= 0.75).all() and (p["contrast"] < 1.25).all()
    assert p["map"].dtype == np.int64 and p["map"].shape == (n, 6)


def test_fixed_seed_reproduces_the_committed_table():
    """Freezes the draw order: any change to what sample_params draws, or in which order, changes this table."""
    t = json.load(open(os.path.join(GOLDEN, "augs_params_seed11.json")))
    p = _params(t["seed"], t["n"], tuple(t["src_hw"]), tuple(t["out_hw"]))
    assert sorted(p) == sorted(t["params"])
    for k, want in t["params"].items():
        got = p[k]
        if got.dtype.kind == "f":
            want = np.array(want, dtype=object)
            want[want == None] = np.nan  # noqa: E711  (JSON has no NaN: stored as null)
            want = want.astype(np.float64)
            assert np.array_equal(got, want, equal_nan=True), k  # floats are stored with repr(): exact
        else:
            assert got.tolist() == want, k


def test_policy_none_is_the_identity_and_takes_explicit_arrays():
    from cerberus_amd import augs

    p = augs.sample_params(2, (10, 12), (6, 8), None, policy=None)
    assert p["map"].tolist() == [[65536, 0, 2 * 65536, 0, 65536, 2 * 65536]] * 2  # the plain centre crop
    assert not p["gauss_k"].any() and not p["median_k"].any() and np.isnan(p["noise_sigma"]).all() and np.isnan(p["hue"]).all()
    q = augs.sample_params(2, (10, 12), (6, 8), None, policy=None, fliplr=[True, False], median_k=[3, 0], hue=[np.nan, 4.0])
    assert q["map"][0].tolist() == [-65536, 0, (2 + 7) * 65536, 0, 65536, 2 * 65536] and q["map"][1].tolist() == p["map"][1].tolist()
    assert q["median_k"].tolist() == [3, 0] and np.isnan(q["hue"][0]) and q["hue"][1] == 4.0
    with pytest.raises(KeyError):
        augs.sample_params(2, (10, 12), (6, 8), None, policy=None, no_such=[1, 2])
    with pytest.raises(ValueError):
        augs.sample_params(2, (10, 12), (16, 8), None, policy=None)


# ---- compose_map ----------------------------------------------------------------------------------------------------------------------------------------
EXACT = [dict(translate=(tx, ty), rotate_deg=rot, fliplr=fl, flipud=fu)
         for tx, ty in ((0, 0), (3, -2), (-5, 4)) for rot in (0, 90, 180, 270, -90) for fl in (False, True) for fu in (False, True)]


@pytest.mark.parametrize("src,out", [((37, 45), (24, 28)), ((20, 20), (20, 20)), ((31, 30), (17, 12))])
def test_integer_folding_equals_quantising_the_composed_float_map(src, out):
    """Whole-pixel translations and rotations by multiples of 90 degrees: every entry of the composed float map times 65536 is an integer (up to
    rounding noise far below 1/2), so folding crop and flips into the quantised integers equals quantising the composed float map."""
    from cerberus_amd import augs

    for kw in EXACT:
        folded = R.compose_map(src, out, **kw)
        assert folded == R.compose_map_float(src, out, **kw), kw
        mine = augs.compose_map(src, out, translate=kw["translate"], rotate=kw["rotate_deg"], fliplr=kw["fliplr"], flipud=kw["flipud"])
        assert mine.tolist() == folded, kw


def test_product_and_restatement_compose_the_same_map_on_random_draws():
    from cerberus_amd import augs

    p = augs.sample_params(32, (130, 70), (100, 66), np.random.RandomState(9))
    for i in range(32):
        want = R.compose_map((130, 70), (100, 66), p["scale"][i], p["shear"][i], p["translate"][i], p["rotate"][i], p["fliplr"][i], p["flipud"][i])
        assert p["map"][i].tolist() == want, i


def test_rot90_and_flips_on_the_restatement():
    a = np.arange(49 * 2, dtype=np.int32).reshape(1, 7, 7, 2)
    for rot, k in ((90, 3), (-90, 1), (180, 2), (0, 0)):
        assert np.array_equal(R.warp(a, [R.compose_map((7, 7), (7, 7), rotate_deg=rot)], (7, 7))[0], np.rot90(a[0], k)), rot
    assert np.array_equal(R.warp(a, [R.compose_map((7, 7), (7, 7), fliplr=True)], (7, 7))[0], a[0, :, ::-1])
    assert np.array_equal(R.warp(a, [R.compose_map((7, 7), (7, 7), flipud=True)], (7, 7))[0], a[0, ::-1])
    assert np.array_equal(R.warp(a, [R.compose_map((7, 7), (3, 5))], (3, 5))[0], a[0, 2:5, 1:6])
