"""NumPy restatement of the nuScenes camera ingest (test infrastructure only): Pillow's 8-bit BILINEAR resize as a pair of 22-bit
fixed-point passes with a uint8 intermediate, the top crop, ToTensor's byte table, and the unpacking of the bit-packed BEV label.
Written from the algorithm's description (Pillow's Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the 8bpc passes), pinned to the
installed Pillow byte for byte by tests/test_nusc_ingest.py and to the reference's own LoadDataTransform by gv_nusc_ingest.npz."""
import math

import numpy as np

BITS = 22

# (H, W) -> (h_resize, w_resize), top crop, n: what each exercises is in the comment
SHAPES = [
    ((37, 53), (11, 17), 3, 1),          # odd W, 7 taps, both borders clipped
    ((20, 31), (33, 47), 0, 1),          # up-scale, 2-3 taps, no crop
    ((64, 48), (64, 20), 5, 2),          # vertical pass skipped
    ((48, 64), (20, 64), 0, 2),          # horizontal pass skipped
    ((9, 16), (9, 16), 2, 1),            # crop only
    ((90, 160), (27, 48), 5, 6),         # the nuScenes ratio at one tenth
    ((200, 121), (61, 40), 7, 3),        # several row bands, last band partial, crop not on a band edge
    ((900, 1600), (270, 480), 46, 1),    # the real shape once
]


def shape_id(s):
    return "%dx%d-%dx%d" % (s[0] + s[1])


def taps(n_in, n_out):
    """-> bounds int32 (n_out, 2) [first source index, tap count], coeffs int32 (n_out, ksize)"""
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = np.float64(1.0) * fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coeffs = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = np.zeros(xmax, dtype=np.float64)
        total = np.float64(0.0)
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * (1.0 / fs))
            k[x] = 1.0 - a if a < 1.0 else 0.0
            total = total + k[x]
        for x in range(xmax):
            v = k[x] / total
            coeffs[xx, x] = int((-0.5 if v < 0 else 0.5) + v * (1 << BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coeffs


def one_pass(img, bounds, coeffs, axis):
    """one resample pass of a uint8 array along `axis`, rounded and clipped to uint8"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + src.shape[1:], dtype=np.uint8)
    for i, (first, count) in enumerate(bounds):
        acc = np.zeros(src.shape[1:], dtype=np.int64)
        for t in range(count):
            acc += src[first + t] * int(coeffs[i, t])
        assert int(acc.max(initial=0)) + (1 << (BITS - 1)) < 2 ** 31        # int32 accumulators suffice
        out[i] = np.clip((acc + (1 << (BITS - 1))) >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8(images, size, top_crop=0):
    """images (n, H, W, 3) uint8, size = (w_resize, h_resize) -> (n, h_resize - top_crop, w_resize, 3) uint8"""
    images = np.asarray(images)
    assert images.dtype == np.uint8 and images.ndim == 4
    wr, hr = size
    out = images
    if images.shape[2] != wr:                       # horizontal first, rounded to bytes
        out = one_pass(out, *taps(images.shape[2], wr), axis=2)
    if images.shape[1] != hr:
        out = one_pass(out, *taps(images.shape[1], hr), axis=1)
    return np.ascontiguousarray(out[:, top_crop:])


def byte_table():
    return np.arange(256, dtype=np.float32) / np.float32(255)


def to_tensor(u8_nhwc):
    """ToTensor of each image: (n, h, w, 3) uint8 -> (n, 3, h, w) fp32 of byte / 255"""
    return np.ascontiguousarray(byte_table()[u8_nhwc].transpose(0, 3, 1, 2))


def resize(images, size, top_crop=0):
    return to_tensor(resize_u8(images, size, top_crop))


def decode_bev(labels, num_classes):
    """(h, w) int32 bit-packed -> (num_classes, h, w) fp32 of 0.0 / 1.0"""
    labels = np.asarray(labels)
    assert labels.dtype == np.int32
    return np.stack([((labels >> c) & 1) for c in range(num_classes)]).astype(np.float32)


def make_images(seed, n, height, width):
    """seeded random bytes; the top third of every image is random 0 / 255 blocks, so that saturation, the rounding of the uint8
    intermediate and the clip all matter"""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(n, height, width, 3)).astype(np.uint8)
    third = max(height // 3, 1)
    bh, bw = max(third // 3, 1), max(width // 7, 1)
    blocks = rng.randint(0, 2, size=(n, (third + bh - 1) // bh, (width + bw - 1) // bw, 3)).astype(np.uint8) * 255
    img[:, :third] = np.repeat(np.repeat(blocks, bh, axis=1), bw, axis=2)[:, :third, :width]
    return img


_CACHE = {}


def case(shape):
    """(images, uint8 result) of one SHAPES row, computed once per process"""
    key = shape_id(shape)
    if key not in _CACHE:
        (hs, ws), (hr, wr), top, n = shape
        img = make_images(sum(shape[0]) * 1000 + sum(shape[1]), n, hs, ws)
        ref = resize_u8(img, (wr, hr), top)
        img.setflags(write=False)
        ref.setflags(write=False)
        _CACHE[key] = (img, ref)
    return _CACHE[key]
