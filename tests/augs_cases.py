"""Inputs shared by tests/test_augs_host.py and tests/test_augs_gpu.py (seeded; nothing here touches the GPU)."""
import numpy as np

NOISE_TOL = 1e-6  # distance of the restatement's pre-floor value from an integer below which a noise pixel may differ by one


def noise_case():
    """33 x 31, N = 4: (img, sigma, per_channel, key) -- shared and per-channel noise, small and large sigma"""
    img = np.random.RandomState(21).randint(0, 256, (4, 33, 31, 3)).astype(np.uint8)
    sigma = np.array([12.75, 5.0, 0.7, 9.25])
    per_channel = np.array([0, 1, 1, 0], np.int32)
    key = np.array([0x0123456789ABCDEF, 7, 0xFFFFFFFF00000001, 1 << 63], np.uint64)
    return img, sigma, per_channel, key


def noise_excluded(pre):
    return np.abs(pre - np.rint(pre)) < NOISE_TOL


def colour_pixels():
    """[1, 1, 343 + 256 + 4096, 3]: the cube {0, 1, 2, 127, 128, 254, 255}^3, all greys, 4096 random pixels"""
    v = np.array([0, 1, 2, 127, 128, 254, 255])
    cube = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    greys = np.repeat(np.arange(256)[:, None], 3, 1)
    rnd = np.random.RandomState(22).randint(0, 256, (4096, 3))
    return np.concatenate([cube, greys, rnd]).astype(np.uint8)[None, None]
