"""The numpy model of the panorama pyramid's rule (tests/pyramid_helpers.py) on hand-made blocks: it is the yardstick of every device
test of pcl_pano_pyramid, so it is pinned here by values worked out by hand from the rule's text (include/piccolo_hip.h)."""
import numpy as np
import pytest

import pyramid_helpers as ph

BLACK = (0, 0, 0)


def one_block(p0, p1, p2, p3):
    """the level-1 pixel of the 2 x 2 image [[p0, p1], [p2, p3]], by both forms of the model"""
    img = np.array([[p0, p1], [p2, p3]], dtype=np.uint8)
    out = ph.next_level(img)
    assert out.shape == (1, 1, 3) and out.dtype == np.uint8
    assert tuple(out[0, 0]) == tuple(ph.block_rule(img.reshape(4, 3)))
    return tuple(int(v) for v in out[0, 0])


def test_counts_zero_to_four():
    a, b, c, d = (10, 20, 30), (30, 40, 50), (50, 60, 70), (70, 80, 90)
    assert one_block(BLACK, BLACK, BLACK, BLACK) == BLACK                       # cnt 0: no data stays no data
    assert one_block(BLACK, a, BLACK, BLACK) == a                               # cnt 1: the pixel itself, wherever it sits
    assert one_block(a, BLACK, BLACK, b) == (20, 30, 40)                        # cnt 2
    assert one_block(a, b, c, BLACK) == (30, 40, 50)                            # cnt 3: 90 / 3, 120 / 3, 150 / 3
    assert one_block(a, b, c, d) == (40, 50, 60)                                # cnt 4
    # the black pixels do not pull the mean down: a naive mean of the cnt 1 block would be (2, 5, 7)
    assert one_block(BLACK, a, BLACK, BLACK) != (2, 5, 7)


def test_ties_round_up_and_the_rest_to_nearest():
    assert one_block((1, 2, 3), (2, 3, 4), BLACK, BLACK) == (2, 3, 4)            # cnt 2: x.5 goes up
    assert one_block((1, 1, 1), (1, 1, 2), (1, 2, 2), (3, 2, 2)) == (2, 2, 2)    # cnt 4: 6/4 = 1.5 -> 2, 6/4 -> 2, 7/4 = 1.75 -> 2
    assert one_block((1, 1, 1), (1, 1, 1), (1, 1, 1), (2, 1, 1)) == (1, 1, 1)    # cnt 4: 5/4 = 1.25 -> 1
    assert one_block((1, 0, 5), (1, 0, 5), (2, 1, 6), BLACK) == (1, 0, 5)        # cnt 3: 4/3 -> 1, 1/3 -> 0, 16/3 = 5.33 -> 5
    assert one_block((1, 0, 5), (2, 1, 6), (2, 1, 6), BLACK) == (2, 1, 6)        # cnt 3: 5/3 = 1.67 -> 2, 2/3 -> 1, 17/3 = 5.67 -> 6
    assert one_block((255, 255, 255), (255, 255, 255), (255, 255, 255), (255, 255, 254)) == (255, 255, 255)    # 1019/4 = 254.75 -> 255: no overflow


def test_a_block_with_data_never_comes_out_black():
    # the fix-up: three data pixels, channel sums (1, 1, 1): (1 + 1) / 3 = 0 on every channel -> every channel holds the largest sum
    assert one_block((1, 0, 0), (0, 1, 0), (0, 0, 1), BLACK) == (1, 1, 1)
    # a non-black block that a naive mean over all four pixels would turn black: (1 + 2) / 4 = 0
    assert one_block(BLACK, BLACK, (0, 0, 1), BLACK) == (0, 0, 1)
    assert one_block((0, 1, 0), BLACK, BLACK, BLACK) == (0, 1, 0)
    # sums below the rounding threshold on SOME channels only: no fix-up, those channels are 0
    assert one_block((1, 0, 0), (1, 0, 0), (0, 0, 1), BLACK) == (1, 0, 0)        # sums (2, 0, 1): (2 + 1) / 3 = 1, 0, (1 + 1) / 3 = 0


def test_black_caps_stay_black_and_a_coarse_pixel_is_black_iff_no_data():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(8, 16, 3), dtype=np.uint8)
    img[rng.random((8, 16)) < 0.5] = 0
    img[:2] = 0
    img[-2:] = 0
    lv1 = ph.next_level(img)
    assert not lv1[0].any() and not lv1[-1].any()
    data = img.any(axis=2).reshape(4, 2, 8, 2).any(axis=(1, 3))
    assert np.array_equal(lv1.any(axis=2), data)
    lv2 = ph.next_level(lv1)
    assert np.array_equal(lv2.any(axis=2), data.reshape(2, 2, 4, 2).any(axis=(1, 3)))


def test_levels_are_cascaded_not_made_from_level_zero():
    # a 4 x 4 block: top-left 2 x 2 holds ONE data pixel of 100, the other three 2 x 2 blocks are full of 20s
    img = np.full((4, 4, 3), 20, dtype=np.uint8)
    img[:2, :2] = 0
    img[0, 1] = 100
    lv1, lv2 = ph.pyramid(img, 2)
    assert [tuple(p) for p in lv1.reshape(4, 3)] == [(100,) * 3, (20,) * 3, (20,) * 3, (20,) * 3]
    assert tuple(lv2[0, 0]) == (40, 40, 40)                                      # (100 + 60 + 2) / 4 from level 1
    direct = (100 + 12 * 20 + 6) // 13                                           # what the 13 data pixels of level 0 would give: 26
    assert direct == 26 and tuple(lv2[0, 0]) != (direct,) * 3
    # and a cascaded fix-up: level 1 is (1,0,0), (0,1,0), (0,0,1), black -> level 2 (1, 1, 1); level 0 directly would give the same
    # three pixels, but through level 1 only
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    img[0, 0], img[1, 3], img[2, 1] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    lv1, lv2 = ph.pyramid(img, 2)
    assert [tuple(p) for p in lv1.reshape(4, 3)] == [(1, 0, 0), (0, 1, 0), (0, 0, 1), BLACK]
    assert tuple(lv2[0, 0]) == (1, 1, 1)


def test_the_vectorised_form_is_the_block_rule_on_every_block():
    rng = np.random.default_rng(11)
    img = rng.integers(0, 4, size=(12, 20, 3), dtype=np.uint8)                   # small levels: plenty of zeros, ties and fix-ups
    img[rng.random((12, 20)) < 0.4] = 0
    lv1 = ph.next_level(img)
    for y in range(6):
        for x in range(10):
            assert tuple(lv1[y, x]) == tuple(ph.block_rule(img[2 * y:2 * y + 2, 2 * x:2 * x + 2].reshape(4, 3))), (y, x)


def test_refusals_and_the_float_image():
    img = np.zeros((8, 12, 3), dtype=np.uint8)
    for levels in (0, 5, 3):                                                    # 12 is no multiple of 8
        with pytest.raises(ValueError):
            ph.pyramid(img, levels)
    assert [lv.shape for lv in ph.pyramid(img, 2)] == [(4, 6, 3), (2, 3, 3)]
    k = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    f = ph.as_float(k)
    assert f.dtype == np.float32 and np.array_equal(f, (k.astype(np.float64) / 255.0).astype(np.float32))    # correctly rounded: via float64
    assert np.array_equal(np.rint(f * np.float32(255.0)).astype(np.uint8), k)


def test_the_planted_image_holds_what_the_device_tests_need():
    for (H, W, levels) in ((12, 20, 2), (16, 32, 4), (48, 80, 4), (272, 528, 4)):
        img = ph.planted_image(H, W, levels, seed=H)
        assert not img[0].any() and not img[-1].any()
        blocks = img.any(axis=2).reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
        assert set(np.unique(blocks)) == {0, 1, 2, 3, 4}
        black = 1.0 - img.any(axis=2).mean()
        assert 0.2 < black < 0.5
        lv = ph.pyramid(img, levels)
        for l, cur, prev in ((1, lv[0], img), (2, lv[1], lv[0])):
            # a fix-up happened at this level: an output (1, 1, 1) whose block sums are (1, 1, 1) over three data pixels
            h, w = cur.shape[:2]
            b = prev.astype(np.int64).reshape(h, 2, w, 2, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, 4, 3)
            fix = ((b != 0).any(axis=3).sum(axis=2) == 3) & (b.sum(axis=2) == 1).all(axis=2)
            assert fix.any(), (H, W, l)
            assert (cur[fix] == 1).all()
