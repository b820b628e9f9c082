"""GPU tests of the depth mask inside shared chains (pcl_gd_run_depth_chain): per-image colour sets of one room, several rooms, rooms x
images.  Every (room, image) must be the depth-masked single chain's — ops.GradientDescent(depth_mask=True) on that room with that image's
colours — bit for bit: loss history, state, winner and leaf rows, on every room's own default grid and on an explicit one, across calls
(the two z-buffer sets) and through the public functions, which now build ONE chain per chain-cap group under cfg.depth_mask."""
import numpy as np
import pytest
import torch

from test_room_images import _per_image_colours, _rgb_of, _starts
from test_room_search import H, W, _cfg, _rooms, _single

pytestmark = pytest.mark.gpu

SIZES = (700, 30_000, 60_000)                # default grids 16 x 32, 32 x 64, 48 x 96; 700 points: fewer steps than chunks; none a multiple of 512
N_ITER = 10
EXPLICIT = dict(depth_res=[64, 128], depth_stride=1, depth_tau=0.05)
GRIDS = {"default": {}, "explicit": EXPLICIT}
GD = dict(lr=0.1, patience=5, factor=0.8)


def _scene():
    """three rooms in one frame, room 1 the FURNISHED room (seed 3) with room 1's colour phase, and three query images: room 1 from
    room_gt_pose(1, 0) and (1, 2), room 2 from (2, 4)"""
    from piccolo_amd import ops, synth
    rooms = _rooms(SIZES)
    xyz, _ = synth.furnished_room(SIZES[1], seed=3)
    rgb = 0.5 + 0.45 * np.sin(xyz.astype(np.float64) @ synth._K.T + synth._PHI + 1.7 * 2 + np.array([0.0, 0.9, 2.1]))
    rooms[1] = (torch.from_numpy((xyz + synth.room_offset(1)[None, :]).astype(np.float32)).cuda(), torch.from_numpy(rgb.astype(np.float32)).cuda())
    imgs = []
    for r, s in ((1, 0), (1, 2), (2, 4)):
        t, ypr = synth.room_gt_pose(r, s)
        cam = ops.transform_cloud(rooms[r][0], torch.from_numpy(t), torch.from_numpy(ypr))
        imgs.append(synth.quantise_like_image_file(ops.make_pano(cam, rooms[r][1], (H, W))))
    return rooms, imgs, xyz


@pytest.fixture(scope="module")
def scene():
    rooms, imgs, furnished_local = _scene()
    return {"shared": rooms, "sets": _per_image_colours(rooms, 3, seed=5), "imgs": imgs, "furnished": furnished_local, "panos": {}, "singles": {}}


def _panos(scene, fmt):
    from piccolo_amd import ops
    if fmt not in scene["panos"]:
        scene["panos"][fmt] = [ops.Pano(im, fmt=fmt) for im in scene["imgs"]]
    return scene["panos"][fmt]


def _clouds(rooms):
    from piccolo_amd import omniloc as po
    from piccolo_amd import ops
    sets = isinstance(rooms[0][1], list)
    return [po.packed_cloud_sets(x, c) if sets else po.packed_cloud(x, c) for x, c in rooms], [ops.quantile_box(x, 0.05) for x, _ in rooms]


def _single_chain(scene, colours, per_image, fmt, grid, r, i, depth=True):
    """(loss history, result) of ops.GradientDescent(depth_mask=True) on room r with image i's colours: computed once, shared by the tests"""
    from piccolo_amd import ops
    key = (colours, per_image, fmt, grid, r, i, depth)
    if key not in scene["singles"]:
        rooms = scene[colours]
        clouds, boxes = _clouds(rooms)
        tr, ro = _starts(3, 3, per_image, seed=5)[r][i]
        one_cloud = ops.Cloud(rooms[r][0], _rgb_of(rooms[r], i), order=clouds[r].order)
        one = ops.GradientDescent(one_cloud, _panos(scene, fmt)[i], tr, ro, boxes[r], depth_mask=depth, **GD, **(GRIDS[grid] if depth else {}))
        scene["singles"][key] = (one.run(N_ITER, history=True), one.result())
    return scene["singles"][key]


def _chain(scene, colours, per_image, fmt, grid, room_ids=(0, 1, 2), image_ids=(0, 1, 2), depth=True):
    from piccolo_amd import ops
    rooms = scene[colours]
    clouds, boxes = _clouds(rooms)
    if colours == "sets" and len(image_ids) != 3:
        raise ValueError("the colour-set clouds of the scene hold three sets")
    starts = _starts(3, 3, per_image, seed=5)
    tr = torch.cat([starts[r][i][0] for r in room_ids for i in image_ids])
    ro = torch.cat([starts[r][i][1] for r in room_ids for i in image_ids])
    panos = [_panos(scene, fmt)[i] for i in image_ids]
    return ops.GradientDescentRoomsImages([(clouds[r], boxes[r]) for r in room_ids], panos, tr, ro, depth_mask=depth, **GD,
                                          **(GRIDS[grid] if depth else {}))


def _assert_equals_singles(scene, hist, res, colours, per_image, fmt, grid, room_ids, image_ids):
    for a, r in enumerate(room_ids):
        for b, i in enumerate(image_ids):
            h1, r1 = _single_chain(scene, colours, per_image, fmt, grid, r, i)
            k = (a * len(image_ids) + b) * per_image
            assert torch.equal(hist[:, k:k + per_image], h1), (r, i)
            assert torch.equal(res[k:k + per_image], r1), (r, i)


@pytest.mark.parametrize("grid", ["default", "explicit"])
@pytest.mark.parametrize("fmt", ["f16", "u8", "f32"])
@pytest.mark.parametrize("per_image", [6, 5])
@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_depth_chain_engine_equals_single_depth_chains(scene, colours, per_image, fmt, grid):
    gd = _chain(scene, colours, per_image, fmt, grid)
    nch, G, fused, grids = gd.plan()
    assert G == (2 if per_image % 2 == 0 else 1) and fused is False
    assert grids == ([(64, 128, 1)] * 3 if grid == "explicit" else [(16, 32, 1), (32, 64, 1), (48, 96, 1)]), grids
    hist = gd.run(N_ITER, history=True)
    assert bool(torch.isfinite(hist).all())
    _assert_equals_singles(scene, hist, gd.result(), colours, per_image, fmt, grid, (0, 1, 2), (0, 1, 2))


@pytest.mark.parametrize("grid", ["default", "explicit"])
@pytest.mark.parametrize("per_image", [6, 5])
def test_one_room_with_colour_sets_and_one_image_with_several_rooms(scene, per_image, grid):
    from piccolo_amd import ops
    # R = 1, colour sets, through the rooms x images engine and through ops.GradientDescent (what omniloc_batch_images builds)
    gd = _chain(scene, "sets", per_image, "f16", grid, room_ids=(1,))
    hist = gd.run(N_ITER, history=True)
    _assert_equals_singles(scene, hist, gd.result(), "sets", per_image, "f16", grid, (1,), (0, 1, 2))
    clouds, boxes = _clouds(scene["sets"])
    starts = _starts(3, 3, per_image, seed=5)
    one = ops.GradientDescent(clouds[1], _panos(scene, "f16")[0], torch.cat([starts[1][i][0] for i in range(3)]),
                              torch.cat([starts[1][i][1] for i in range(3)]), boxes[1], depth_mask=True, **GD, **GRIDS[grid])
    one.set_pano_groups(_panos(scene, "f16"))
    h1 = one.run(N_ITER, history=True)
    assert torch.equal(h1, hist) and torch.equal(one.result(), gd.result())
    # I = 1: ops.GradientDescentRooms, and the rooms x images engine with one image
    clouds, boxes = _clouds(scene["shared"])
    tr, ro = torch.cat([starts[r][0][0] for r in range(3)]), torch.cat([starts[r][0][1] for r in range(3)])
    gr = ops.GradientDescentRooms(list(zip(clouds, boxes)), _panos(scene, "f16")[0], tr, ro, depth_mask=True, **GD, **GRIDS[grid])
    assert len(gr.plan()) == 4 and gr.plan()[2] is False
    hr = gr.run(N_ITER, history=True)
    _assert_equals_singles(scene, hr, gr.result(), "shared", per_image, "f16", grid, (0, 1, 2), (0,))
    gi = _chain(scene, "shared", per_image, "f16", grid, image_ids=(0,))
    assert torch.equal(gi.run(N_ITER, history=True), hr) and torch.equal(gi.result(), gr.result())
    # one room, one image: pcl_gd_run itself
    g11 = _chain(scene, "shared", per_image, "f16", grid, room_ids=(2,), image_ids=(1,))
    h11 = g11.run(N_ITER, history=True)
    _assert_equals_singles(scene, h11, g11.result(), "shared", per_image, "f16", grid, (2,), (1,))


@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_continuing_a_depth_chain_equals_one_call(scene, colours):
    """run(4) then run(6) against run(10): both z-buffer sets are scratch, every call fills the set its first iteration reads"""
    whole = _chain(scene, colours, 6, "f16", "default")
    h = whole.run(N_ITER, history=True)
    parts = _chain(scene, colours, 6, "f16", "default")
    h4, h6 = parts.run(4, history=True), parts.run(6, history=True)
    assert torch.equal(torch.cat([h4, h6]), h) and torch.equal(parts.result(), whole.result())
    odd = _chain(scene, colours, 6, "f16", "default")                      # (an odd first call: the second call starts on set 0 again)
    assert torch.equal(torch.cat([odd.run(3, history=True), odd.run(7, history=True)]), h) and torch.equal(odd.result(), whole.result())
    _assert_equals_singles(scene, h, whole.result(), colours, 6, "f16", "default", (0, 1, 2), (0, 1, 2))


def test_the_mask_changes_the_furnished_rooms_losses(scene):
    """not vacuous: 18-24 % of the furnished room's points are hidden from its two query poses, and the masked chain's losses differ"""
    from piccolo_amd import synth
    for s in (0, 2):
        hidden = synth.occluded_by_furniture(scene["furnished"], synth.gt_pose(s)[0]).mean()
        assert 0.15 <= hidden <= 0.30, (s, hidden)
    masked = _chain(scene, "shared", 6, "f16", "default", image_ids=(0, 1)).run(N_ITER, history=True)
    plain = _chain(scene, "shared", 6, "f16", "default", image_ids=(0, 1), depth=False).run(N_ITER, history=True)
    for i in range(2):                                 # room 1's columns of image i
        k = (1 * 2 + i) * 6
        assert not torch.equal(masked[0, k:k + 6], plain[0, k:k + 6]), i       # (the same poses: the mask alone)
        assert not torch.equal(masked[:, k:k + 6], plain[:, k:k + 6]), i


def test_colour_sets_with_the_depth_mask_no_longer_raise(scene):
    from piccolo_amd import ops
    clouds, boxes = _clouds(scene["sets"])
    assert clouds[2].color_sets == 3
    starts = _starts(3, 3, 4, seed=9)
    gd = ops.GradientDescent(clouds[2], _panos(scene, "u8")[2], torch.cat([starts[2][i][0] for i in range(3)]),
                             torch.cat([starts[2][i][1] for i in range(3)]), boxes[2], depth_mask=True, **GD)
    assert bool(torch.isfinite(gd.run(2, history=True)).all())
    with pytest.raises(ValueError):                    # (candidates that do not split over the sets are still refused)
        ops.GradientDescent(clouds[2], _panos(scene, "u8")[2], starts[2][0][0][:4], starts[2][0][1][:4], boxes[2], depth_mask=True, **GD)


# ---------------------------------------------------------------- the public functions

MANY = [2_000 + 997 * r for r in range(40)]                  # across the 32-room chain cap: chains of 32 and 8 rooms


@pytest.fixture(scope="module")
def many():
    from test_room_search import _query
    base = _rooms(MANY, seed=1)
    return {"shared": base, "sets": _per_image_colours(base, 2, seed=3), "imgs": [_query(base, 17, 3)[0], _query(base, 4, 8)[0]]}


class _Counters:
    """counts the chain builders and everything a per-room / per-image fallback would go through while the call under test runs"""

    def __init__(self, monkeypatch):
        from piccolo_amd import omniloc as po
        self.calls = {"rooms": [], "rooms_images": [], "refine": 0}
        real_r, real_ri, real_ref = po._rooms_chain, po._rooms_images_chain, po._refine
        monkeypatch.setattr(po, "_rooms_chain", lambda img, rooms, *a, **k: self.calls["rooms"].append(len(rooms)) or real_r(img, rooms, *a, **k))
        monkeypatch.setattr(po, "_rooms_images_chain",
                            lambda imgs, rooms, *a, **k: self.calls["rooms_images"].append((len(imgs), len(rooms))) or real_ri(imgs, rooms, *a, **k))

        def refine(*a, **k):
            self.calls["refine"] += 1
            return real_ref(*a, **k)
        monkeypatch.setattr(po, "_refine", refine)


@pytest.mark.parametrize("batch_mode", [True, False])
def test_omniloc_batch_rooms_builds_one_depth_chain_per_cap_group(many, monkeypatch, batch_mode):
    from piccolo_amd import omniloc as po
    from test_room_search import _starts as starts_rooms
    rooms, img = many["shared"], many["imgs"][0]
    cfg = _cfg(num_input=4, num_iter=6, depth_mask=True)
    starts = starts_rooms(40, 4, seed=6)
    tr_m, ro_m = [t.clone() for t, _ in starts], [r.clone() for _, r in starts]
    with monkeypatch.context() as m:
        c = _Counters(m)
        got = po.omniloc_batch_rooms(img, rooms, tr_m, ro_m, cfg, batch_mode=batch_mode)
    assert c.calls == {"rooms": [32, 8], "rooms_images": [], "refine": 0}, c.calls
    for r, room in enumerate(rooms):
        tr, ro = starts[r][0].clone(), starts[r][1].clone()
        want = _single(img, room, tr, ro, cfg, batch_mode)
        for k in range(3):
            assert torch.equal(got[r][k], want[k]), (r, k)
        assert torch.equal(tr_m[r], tr) and torch.equal(ro_m[r], ro), r


@pytest.mark.parametrize("batch_mode", [True, False])
@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_omniloc_batch_rooms_images_builds_one_depth_chain_per_cap_group(many, monkeypatch, colours, batch_mode):
    from piccolo_amd import omniloc as po
    rooms, imgs = many[colours], many["imgs"]
    cfg = _cfg(num_input=4, num_iter=6, depth_mask=True)
    starts = _starts(40, 2, 4, seed=6)
    tr_m = [[s[0].clone() for s in row] for row in starts]
    ro_m = [[s[1].clone() for s in row] for row in starts]
    with monkeypatch.context() as m:
        c = _Counters(m)
        got = po.omniloc_batch_rooms_images(imgs, rooms, tr_m, ro_m, cfg, batch_mode=batch_mode)
    assert c.calls == {"rooms": [], "rooms_images": [(2, 32), (2, 8)], "refine": 0}, c.calls
    for r, room in enumerate(rooms):
        for i in range(2):
            tr, ro = starts[r][i][0].clone(), starts[r][i][1].clone()
            want = _single(imgs[i], (room[0], _rgb_of(room, i)), tr, ro, cfg, batch_mode)
            for k in range(3):
                assert torch.equal(got[r][i][k], want[k]), (r, i, k)
            assert torch.equal(tr_m[r][i], tr) and torch.equal(ro_m[r][i], ro), (r, i)


@pytest.mark.parametrize("batch_mode", [True, False])
def test_omniloc_batch_images_shares_one_depth_chain_between_colour_sets(scene, monkeypatch, batch_mode):
    from piccolo_amd import omniloc as po
    xyz, cols = scene["sets"][1]
    imgs = scene["imgs"]
    cfg = _cfg(num_iter=N_ITER, depth_mask=True)
    starts = _starts(3, 3, 6, seed=5)[1]
    tr_m, ro_m = [s[0].clone() for s in starts], [s[1].clone() for s in starts]
    with monkeypatch.context() as m:
        c = _Counters(m)
        got = po.omniloc_batch_images(imgs, xyz, cols, tr_m, ro_m, cfg, batch_mode=batch_mode)
    assert c.calls == {"rooms": [], "rooms_images": [], "refine": 1}, c.calls           # one chain for the three images, not one each
    for i in range(3):
        tr, ro = starts[i][0].clone(), starts[i][1].clone()
        want = _single(imgs[i], (xyz, cols[i]), tr, ro, cfg, batch_mode)
        for k in range(3):
            assert torch.equal(got[i][k], want[k]), (i, k)
        assert torch.equal(tr_m[i], tr) and torch.equal(ro_m[i], ro), i
