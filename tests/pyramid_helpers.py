"""The numpy model of the panorama pyramid's rule (include/piccolo_hip.h, pcl_pano_pyramid): uint8 levels in, uint8 levels out, one
level at a time.  Written from the rule's text, in int64, one block at a time where that is clearer than fast."""
import numpy as np


def block_rule(pixels):
    """The rule on the pixels of ONE 2 x 2 block: (4, 3) integer levels -> (3,) levels."""
    px = np.asarray(pixels, dtype=np.int64).reshape(4, 3)
    data = px[(px != 0).any(axis=1)]                 # black = all three channels 0 = no data
    cnt = len(data)
    if cnt == 0:
        return np.zeros(3, dtype=np.int64)
    sums = data.sum(axis=0)
    out = (sums + cnt // 2) // cnt                   # round to nearest, ties up
    if not out.any():
        out = (sums == sums.max()).astype(np.int64)  # a block with data never comes out black
    return out


def next_level(lv):
    """(h, w, 3) uint8 with even h and w -> (h / 2, w / 2, 3) uint8 by aligned 2 x 2 blocks (vectorised block_rule)."""
    lv = np.asarray(lv)
    assert lv.dtype == np.uint8 and lv.ndim == 3 and lv.shape[2] == 3 and lv.shape[0] % 2 == 0 and lv.shape[1] % 2 == 0
    h, w = lv.shape[0] // 2, lv.shape[1] // 2
    b = lv.astype(np.int64).reshape(h, 2, w, 2, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, 4, 3)
    cnt = (b != 0).any(axis=3).sum(axis=2)           # (black pixels add nothing to the sums)
    sums = b.sum(axis=2)
    c = np.maximum(cnt, 1)[..., None]
    out = (sums + c // 2) // c
    fix = (cnt > 0) & ~out.any(axis=2)
    out[fix] = (sums[fix] == sums[fix].max(axis=1, keepdims=True)).astype(np.int64)
    out[cnt == 0] = 0
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def pyramid(lv0, levels):
    """[level 1, ..., level `levels`] of the uint8 image lv0, cascaded: level l from level l - 1."""
    if not 1 <= levels <= 4 or lv0.shape[0] % (1 << levels) or lv0.shape[1] % (1 << levels):
        raise ValueError("levels 1..4, H and W multiples of 2^levels")
    out, cur = [], lv0
    for _ in range(levels):
        cur = next_level(cur)
        out.append(cur)
    return out


def as_float(lv):
    """the float image of uint8 levels: the correctly rounded fp32 quotient k / 255"""
    return (lv.astype(np.float32) / np.float32(255.0)).astype(np.float32)


def planted_image(H, W, levels, seed):
    """(H, W, 3) uint8 test image: random levels, about 30 % black pixels, blocks of every cnt, the (1, 1, 1) fix-up case at level 1 and —
    where the image has a second level — at level 2, black top and bottom rows."""
    rng = np.random.default_rng(seed)
    lv = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    lv[rng.random((H, W)) < 0.3] = 0
    # whole 2 x 2 blocks with cnt = 0..4 data pixels, wherever they fit
    by, bx = H // 2, W // 2
    for i, cnt in enumerate(range(5)):
        y, x = 2 * ((1 + i) % by), 2 * ((2 * i + 1) % bx)
        blk = rng.integers(1, 256, size=(2, 2, 3), dtype=np.uint8)
        blk.reshape(4, 3)[cnt:] = 0
        lv[y:y + 2, x:x + 2] = blk
    # the fix-up at level 1: three data pixels with channel sums (1, 1, 1)
    y, x = 2 * (by // 2), 2 * (bx // 2)
    lv[y:y + 2, x:x + 2] = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [0, 0, 0]]], dtype=np.uint8)
    if levels >= 2:
        # ... and at level 2: a 4 x 4 block whose level-1 pixels are (1,0,0), (0,1,0), (0,0,1), black — each made from one data pixel
        y, x = 4 * ((H // 4) // 2), 4 * (((W // 4) + 1) // 2 - 1) if W // 4 > 1 else 0
        blk = np.zeros((4, 4, 3), dtype=np.uint8)
        blk[0, 0] = (1, 0, 0); blk[1, 3] = (0, 1, 0); blk[2, 1] = (0, 0, 1)
        if (y, x) == (4 * ((2 * (by // 2)) // 4), 4 * ((2 * (bx // 2)) // 4)):      # (do not overwrite the level-1 plant: move one block on)
            x = (x + 4) % (4 * (W // 4))
        lv[y:y + 4, x:x + 4] = blk
    if H > 2:
        lv[0] = 0
        lv[-1] = 0
    return lv
