"""Numpy restatement of the MC-dropout factor stream (csrc/dropout.hip), written from its definition on oracle.hua's Philox:

    counter (c >> 2, site, sample, (uint32) image id),  key ((uint32) seed ^ 0x44524F50, seed >> 32),  word c & 3,  u = u01(word)
    factor = u > rate ? fl(1 / (1 - rate)) : 0        (fp32)
"""
import numpy as np

from oracle.hua import _u01, philox4x32

KEY_TAG = 0x44524F50


def keep_scale(rate):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def masks_numpy(image_ids, site_channels, rate, seed, sample):
    """-> float32 [B, T], T = sum(site_channels): row b holds the factors of image_ids[b], site after site"""
    k0, k1 = (seed & 0xFFFFFFFF) ^ KEY_TAG, (seed >> 32) & 0xFFFFFFFF
    rows = []
    for img in image_ids:
        row = []
        for s, C in enumerate(site_channels):
            c = np.arange(C, dtype=np.uint32)
            words = philox4x32(c >> np.uint32(2), np.uint32(s), np.uint32(sample), np.uint32(int(img) & 0xFFFFFFFF), k0, k1)
            u = _u01(np.choose(c & np.uint32(3), words))
            row.append(np.where(u > np.float32(rate), keep_scale(rate), np.float32(0.0)).astype(np.float32))
        rows.append(np.concatenate(row))
    return np.stack(rows)
