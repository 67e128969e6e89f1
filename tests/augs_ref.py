"""Restatement of the training augmentations of include/cerberus_hip.h ("training augmentations") in numpy integers and float64.

Written from the header's text, not from csrc/augs.hip, and independent of cerberus_amd.augs: tests/test_augs_host.py pins it to the published known
answers of tests/golden/augs_documented.json and tests/test_augs_gpu.py compares the kernels with it.  Arrays are [N, H, W, 3] uint8 images and
[N, H, W, C] int32 annotations; per-sample parameters are sequences of N entries."""
import numpy as np

GAUSS = {1: [1], 3: [1, 2, 1], 5: [1, 4, 6, 4, 1]}
MASK32 = 0xFFFFFFFF


# ---- Philox4x32-10, twice ---------------------------------------------------------------------------------------------------------------------------
def philox_scalar(counter, key):
    """counter: 4 ints, key: 2 ints (32-bit words) -> 4 ints; plain Python integers."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return [c0, c1, c2, c3]


def philox_vec(c0, c1, c2, c3, k0, k1):
    """The same over numpy uint64 arrays holding 32-bit words (products of two 32-bit words fit 64 bits)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1, c2, c3


# ---- warp -------------------------------------------------------------------------------------------------------------------------------------------
def _translate(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def forward_matrix(src_hw, scale=(1.0, 1.0), shear_deg=0.0, translate=(0.0, 0.0), rotate_deg=0.0):
    """M = T(c + t) R(theta) Shear_x(phi) S(sx, sy) T(-c) in (x, y) coordinates."""
    H, W = src_hw
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    th, ph = np.deg2rad(rotate_deg), np.deg2rad(shear_deg)
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    Sh = np.array([[1.0, np.tan(ph), 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    S = np.diag([float(scale[0]), float(scale[1]), 1.0])
    return _translate(cx + translate[0], cy + translate[1]) @ R @ Sh @ S @ _translate(-cx, -cy)


def invert_affine(M):
    a, b, c = M[0]
    d, e, f = M[1]
    det = a * e - b * d
    return np.array([[e / det, -b / det, (b * f - c * e) / det], [-d / det, a / det, (c * d - a * f) / det], [0.0, 0.0, 1.0]])


def quantise(Minv):
    return [int(np.rint(m * 65536.0)) for m in (Minv[0, 0], Minv[0, 1], Minv[0, 2], Minv[1, 0], Minv[1, 1], Minv[1, 2])]


def compose_map(src_hw, out_hw, scale=(1.0, 1.0), shear_deg=0.0, translate=(0.0, 0.0), rotate_deg=0.0, fliplr=False, flipud=False):
    """The six Q16 integers of one sample: quantise the inverse, then fold crop and flips in integers."""
    H, W = src_hw
    h, w = out_hw
    A, B, C, D, E, F = quantise(invert_affine(forward_matrix(src_hw, scale, shear_deg, translate, rotate_deg)))
    oy, ox = (H - h) // 2, (W - w) // 2
    C, F = C + A * ox + B * oy, F + D * ox + E * oy
    if fliplr:
        C, F = C + A * (w - 1), F + D * (w - 1)
        A, D = -A, -D
    if flipud:
        C, F = C + B * (h - 1), F + E * (h - 1)
        B, E = -B, -E
    return [A, B, C, D, E, F]


def compose_map_float(src_hw, out_hw, scale=(1.0, 1.0), shear_deg=0.0, translate=(0.0, 0.0), rotate_deg=0.0, fliplr=False, flipud=False):
    """The other order: crop and flips composed as FLOAT matrices onto the inverse, quantised afterwards (equal to compose_map where that is exact)."""
    H, W = src_hw
    h, w = out_hw
    Minv = invert_affine(forward_matrix(src_hw, scale, shear_deg, translate, rotate_deg))
    Minv = Minv @ _translate(float((W - w) // 2), float((H - h) // 2))
    if fliplr:
        Minv = Minv @ np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    if flipud:
        Minv = Minv @ np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]])
    return quantise(Minv)


def warp(arr, maps, out_hw):
    """arr [N, H, W, C] (any integer dtype), maps [N][6] -> [N, h, w, C]; nearest neighbour, 0 outside."""
    arr = np.asarray(arr)
    N, H, W, C = arr.shape
    h, w = out_hw
    out = np.zeros((N, h, w, C), arr.dtype)
    v, u = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    for i in range(N):
        A, B, Cc, D, E, F = (int(x) for x in maps[i])
        xs = (A * u + B * v + Cc + 32768) >> 16
        ys = (D * u + E * v + F + 32768) >> 16
        ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        out[i][ok] = arr[i][ys[ok], xs[ok]]
    return out


# ---- blurs ------------------------------------------------------------------------------------------------------------------------------------------
def _window(img, ky, kx):
    """[ky, kx, H, W, 3] taps with replicated borders"""
    H, W = img.shape[:2]
    ys = np.clip(np.arange(H)[None, :] + np.arange(ky)[:, None] - ky // 2, 0, H - 1)
    xs = np.clip(np.arange(W)[None, :] + np.arange(kx)[:, None] - kx // 2, 0, W - 1)
    return img[ys[:, None, :, None], xs[None, :, None, :]]


def gaussian_blur(img, kx, ky):
    img = np.asarray(img)
    out = np.empty_like(img)
    for i in range(img.shape[0]):
        wx, wy = np.array(GAUSS[int(kx[i])], np.int64), np.array(GAUSS[int(ky[i])], np.int64)
        total = int(wx.sum() * wy.sum())
        shift = total.bit_length() - 1
        assert 1 << shift == total
        half = (1 << (shift - 1)) if shift else 0
        taps = _window(img[i], len(wy), len(wx)).astype(np.int64)
        acc = (taps * wy[:, None, None, None, None] * wx[None, :, None, None, None]).sum((0, 1))
        out[i] = (acc + half) >> shift
    return out


def median_blur(img, k):
    img = np.asarray(img)
    out = np.empty_like(img)
    for i in range(img.shape[0]):
        kk = int(k[i])
        taps = _window(img[i], kk, kk).reshape((kk * kk,) + img.shape[1:])
        out[i] = np.sort(taps, axis=0)[kk * kk // 2]
    return out


# ---- noise ------------------------------------------------------------------------------------------------------------------------------------------
def gaussian_noise(img, sigma, per_channel, key):
    """-> (out uint8, pre float64): pre = p + sigma z + 0.5, the value before the floor (the GPU test's exclusion rule reads it)."""
    img = np.asarray(img)
    N, H, W, _ = img.shape
    q = np.arange(H * W, dtype=np.uint64)
    out = np.empty_like(img)
    pre = np.empty(img.shape, np.float64)
    two_pi = 6.283185307179586
    for i in range(N):
        kk = int(key[i])
        r0, r1, r2, r3 = philox_vec(q & np.uint64(MASK32), q >> np.uint64(32), np.zeros_like(q), np.zeros_like(q), kk & MASK32, kk >> 32)
        u1, u2 = (r0.astype(np.float64) + 1.0) * 2.0 ** -32, r1.astype(np.float64) * 2.0 ** -32
        u3, u4 = (r2.astype(np.float64) + 1.0) * 2.0 ** -32, r3.astype(np.float64) * 2.0 ** -32
        rad, ang = np.sqrt(-2.0 * np.log(u1)), two_pi * u2
        z0, z1, z2 = rad * np.cos(ang), rad * np.sin(ang), np.sqrt(-2.0 * np.log(u3)) * np.cos(two_pi * u4)
        z = np.stack([z0, z1, z2] if per_channel[i] else [z0, z0, z0], -1).reshape(H, W, 3)
        pre[i] = img[i].astype(np.float64) + float(sigma[i]) * z + 0.5
        out[i] = np.clip(np.floor(pre[i]), 0, 255).astype(np.uint8)
    return out, pre


# ---- colour -----------------------------------------------------------------------------------------------------------------------------------------
def _per_sample(img, values, fn):
    img = np.asarray(img)
    out = img.copy()
    for i in range(img.shape[0]):
        if np.isfinite(values[i]):
            out[i] = fn(img[i], float(values[i]), i)
    return out


def _store_u8(x):
    return np.clip(x, 0, 255).astype(np.uint8)  # float64 -> uint8 truncates


def grey(img):
    p = np.asarray(img).astype(np.int64)
    return (4899 * p[..., 0] + 9617 * p[..., 1] + 1868 * p[..., 2] + 8192) >> 14


def brightness(img, values):
    return _per_sample(img, values, lambda a, v, i: _store_u8(a.astype(np.float64) + v))


def saturation(img, values):
    def one(a, v, i):
        s = 1.0 + v
        return _store_u8(a.astype(np.float64) * s + (grey(a).astype(np.float64) * (1.0 - s))[..., None])

    return _per_sample(img, values, one)


def rgb_to_hsv(img):
    p = np.asarray(img).astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    V = p.max(-1)
    d = V - p.min(-1)
    S = np.where(V == 0, 0, (510 * d + V) // np.maximum(2 * V, 1))
    hnum = np.where(V == R, G - B, np.where(V == G, (B - R) + 2 * d, (R - G) + 4 * d))
    Hh = np.where(d == 0, 0, (60 * hnum + d) // np.maximum(2 * d, 1))  # numpy's // floors
    Hh = np.where(Hh < 0, Hh + 180, Hh)
    Hh = np.where(Hh >= 180, Hh - 180, Hh)
    return np.stack([Hh, S, V], -1)


def hsv_to_rgb(hsv):
    hsv = np.asarray(hsv).astype(np.float64)
    s, v, hh = hsv[..., 1] / 255.0, hsv[..., 2], hsv[..., 0] / 30.0
    i = np.floor(hh)
    f = hh - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    sec = i.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(hsv.shape, np.float64)
    for k, rgb in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(sec == k, rgb[c], out[..., c])
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def hue(img, values):
    def one(a, v, i):
        hsv = rgb_to_hsv(a)
        r = np.fmod(hsv[..., 0].astype(np.float64) + v, 180.0)
        r = np.where(r < 0.0, r + 180.0, r)
        hsv[..., 0] = np.trunc(r).astype(np.int64)
        return hsv_to_rgb(hsv)

    return _per_sample(img, values, one)


def channel_sums(img):
    return np.asarray(img).astype(np.int64).sum((1, 2))


def contrast(img, values):
    sums = channel_sums(img)
    npx = float(np.asarray(img).shape[1] * np.asarray(img).shape[2])
    return _per_sample(img, values, lambda a, v, i: _store_u8(a.astype(np.float64) * v + (sums[i].astype(np.float64) / npx) * (1.0 - v)))
