"""GPU tests of the room search over several panoramas (ABI 12): I images x R rooms in one launch chain.  Every (room, image) result must
be the single-room, single-image refinement's, bit for bit — state, loss history, winner and the leaf rows written back — with shared
colours and with per-image colour sets, whatever the fuse / graph / batch-mode choice, across the 32-room chain cap and through the
depth-mask fallback; end to end, localize_images_in_rooms must equal localize_in_rooms per image and the Stanford harness with
room_search_images must write the table it writes one image at a time."""
import numpy as np
import pytest
import torch

from conftest import Cfg
from room_helpers import image_starts as _starts, per_image_colours as _per_image_colours
from test_room_search import FUSED_SIZES, H, INIT, SIZES, W, _cfg, _query, _rooms, _single, _write_rooms_tree  # noqa: F401

pytestmark = pytest.mark.gpu


def _queries(rooms, nimages, seed):
    """image i shows room i mod R (from its own shared-colour cloud)"""
    return [_query(rooms, i % len(rooms), seed + i)[0] for i in range(nimages)]


def _rgb_of(room, i):
    return room[1][i] if isinstance(room[1], list) else room[1]


def _compare(imgs, rooms, starts, cfg, batch_mode=True):
    """omniloc_batch_rooms_images against one single-room single-image call per (room, image): t, R, loss and the leaf rows, bit for bit"""
    from piccolo_amd import omniloc as po
    R, I = len(rooms), len(imgs)
    tr_m = [[starts[r][i][0].clone() for i in range(I)] for r in range(R)]
    ro_m = [[starts[r][i][1].clone() for i in range(I)] for r in range(R)]
    got = po.omniloc_batch_rooms_images(imgs, rooms, tr_m, ro_m, cfg, batch_mode=batch_mode)
    assert len(got) == R and all(len(g) == I for g in got)
    for r, room in enumerate(rooms):
        for i in range(I):
            tr, ro = starts[r][i][0].clone(), starts[r][i][1].clone()
            want = _single(imgs[i], (room[0], _rgb_of(room, i)), tr, ro, cfg, batch_mode)
            for k in range(3):
                assert torch.equal(got[r][i][k], want[k]), (r, i, k, got[r][i][k], want[k])
            assert torch.equal(tr_m[r][i], tr) and torch.equal(ro_m[r][i], ro), (r, i)
    return got


@pytest.mark.parametrize("per_image_colours", [False, True])
@pytest.mark.parametrize("batch_mode", [True, False])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("graph", [True, False])
def test_rooms_images_chain_equals_single_calls_bit_for_bit(batch_mode, fuse, graph, per_image_colours):
    base = _rooms(SIZES)
    rooms = _per_image_colours(base, 3) if per_image_colours else base
    cfg = _cfg(gd_fuse=fuse, gd_graph=graph)
    _compare(_queries(base, 3, 5), rooms, _starts(3, 3, 6), cfg, batch_mode)
    if graph:                                         # a second group of images through the cached engine (replay, new poses, panoramas, colours)
        rooms2 = _per_image_colours(base, 3, seed=50) if per_image_colours else base
        _compare(_queries(base, 3, 9), rooms2, _starts(3, 3, 6, seed=11), cfg, batch_mode)


def _engine_against_singles(rooms, imgs, starts, per_image, fuse, n_iter, expect_fused=None):
    """ops.GradientDescentRoomsImages: loss history and final state of every (room, image) against ops.GradientDescent of it alone"""
    from piccolo_amd import ops
    from piccolo_amd import omniloc as po
    R, I = len(rooms), len(imgs)
    sets = isinstance(rooms[0][1], list)
    panos = [ops.Pano(im, fmt="f16") for im in imgs]
    clouds = [po.packed_cloud_sets(x, c) if sets else po.packed_cloud(x, c) for x, c in rooms]
    boxes = [ops.quantile_box(x, 0.05) for x, _ in rooms]
    tr = torch.cat([starts[r][i][0] for r in range(R) for i in range(I)])
    ro = torch.cat([starts[r][i][1] for r in range(R) for i in range(I)])
    gd = ops.GradientDescentRoomsImages(list(zip(clouds, boxes)), panos, tr, ro, lr=0.1, patience=5, factor=0.8, fuse=fuse)
    nch, G, fused = gd.plan()
    assert G == (2 if per_image % 2 == 0 else 1)
    assert fused == (fuse is None and sum(c * I * per_image // G for c in nch) <= 1024)
    if expect_fused is not None:
        assert fused is expect_fused, (nch, G, fused)
    hist = gd.run(n_iter, history=True)
    res = gd.result()
    for r in range(R):
        for i in range(I):
            one_cloud = ops.Cloud(rooms[r][0], _rgb_of(rooms[r], i), order=clouds[r].order)
            one = ops.GradientDescent(one_cloud, panos[i], starts[r][i][0], starts[r][i][1], boxes[r], lr=0.1, patience=5, factor=0.8, fuse=fuse)
            h1 = one.run(n_iter, history=True)
            k = (r * I + i) * per_image
            assert torch.equal(hist[:, k:k + per_image], h1), (r, i)
            assert torch.equal(res[k:k + per_image], one.result()), (r, i)
    return hist, res


@pytest.mark.parametrize("per_image_colours", [False, True])
@pytest.mark.parametrize("fuse", [None, False])
def test_rooms_images_engine_history_equals_single_histories(fuse, per_image_colours):
    base = _rooms(SIZES, seed=4)
    rooms = _per_image_colours(base, 3, seed=2) if per_image_colours else base
    _engine_against_singles(rooms, _queries(base, 3, 2), _starts(3, 3, 6, seed=5), 6, fuse, 31)


SMALL_SIZES = (700, 6_000, 20_000)           # 3 images x 6 candidates: few enough blocks for one launch per iteration


@pytest.mark.parametrize("per_image_colours", [False, True])
def test_fused_rooms_images_chain_equals_the_two_launch_form_and_the_single_calls(per_image_colours):
    base = _rooms(SMALL_SIZES, seed=9)
    rooms = _per_image_colours(base, 3, seed=4) if per_image_colours else base
    imgs = _queries(base, 3, 6)
    starts = _starts(3, 3, 6, seed=13)
    out = {}
    for fuse in (None, False):
        for n_iter in (1, 2, 31):                      # (the fused form's first, second and an odd number of launches)
            out[fuse, n_iter] = _engine_against_singles(rooms, imgs, starts, 6, fuse, n_iter, expect_fused=fuse is None)
    for n_iter in (1, 2, 31):
        assert torch.equal(out[None, n_iter][0], out[False, n_iter][0]) and torch.equal(out[None, n_iter][1], out[False, n_iter][1]), n_iter
    for fuse in (True, False):
        for graph in (True, False):
            for batch_mode in (True, False):
                _compare(imgs, rooms, starts, _cfg(gd_fuse=fuse, gd_graph=graph), batch_mode)


@pytest.mark.parametrize("per_image_colours", [False, True])
def test_odd_candidates_one_image_and_one_room(per_image_colours):
    base = _rooms((5_000, 90_000, 166_667), seed=7)
    rooms = _per_image_colours(base, 3, seed=6) if per_image_colours else base
    imgs = _queries(base, 3, 4)
    _compare(imgs, rooms, _starts(3, 3, 5, seed=2), _cfg(num_input=5))                 # per_image 5: one pose per block (G = 1)
    _engine_against_singles(rooms, imgs, _starts(3, 3, 5, seed=2), 5, None, 12)
    one_img = [(x, c[:1] if isinstance(c, list) else c) for x, c in rooms]
    _compare(imgs[:1], one_img, _starts(3, 1, 6, seed=8), _cfg())                       # I = 1 is omniloc_batch_rooms
    _compare(imgs, rooms[1:2], _starts(1, 3, 6, seed=8), _cfg())                        # R = 1: a chain of one room
    _engine_against_singles(rooms[1:2], imgs, _starts(1, 3, 6, seed=8), 6, None, 12)
    _engine_against_singles(one_img, imgs[:1], _starts(3, 1, 6, seed=8), 6, None, 12)   # I = 1 through the engine: pcl_gd_run_rooms


def test_more_rooms_than_one_chain_takes():
    sizes = [2_000 + 997 * r for r in range(33)]
    base = _rooms(sizes, seed=1)
    imgs = [_query(base, 17, 3)[0], _query(base, 4, 8)[0]]
    cfg = _cfg(num_input=4, num_iter=12)
    _compare(imgs, base, _starts(33, 2, 4, seed=6), cfg)
    _compare(imgs, _per_image_colours(base, 2, seed=3), _starts(33, 2, 4, seed=6), cfg)


def test_images_beyond_the_colour_set_limit_go_in_groups(monkeypatch):
    """a room that holds at most 2 colour sets: 3 images with their own colours run as a chain of 2 images and one of 1, same results"""
    from piccolo_amd import omniloc as po
    from piccolo_amd import ops
    base = _rooms(SIZES, seed=12)
    rooms = _per_image_colours(base, 3, seed=8)
    monkeypatch.setattr(ops, "max_color_sets", lambda n: 2)
    assert po.color_set_groups(SIZES[-1], 3) == [2, 1]
    chains = []
    real = po._rooms_images_chain
    monkeypatch.setattr(po, "_rooms_images_chain", lambda imgs, *a, **k: chains.append(len(imgs)) or real(imgs, *a, **k))
    _compare(_queries(base, 3, 7), rooms, _starts(3, 3, 6, seed=21), _cfg())
    assert chains == [2], chains                       # (the group of one image is omniloc_batch_rooms)
    # shared colours have no such limit: one chain of all three
    del chains[:]
    _compare(_queries(base, 3, 7), base, _starts(3, 3, 6, seed=21), _cfg())
    assert chains == [3], chains


def test_chains_too_large_to_gain_run_one_chain_per_image(monkeypatch):
    from piccolo_amd import omniloc as po
    base = _rooms(SIZES, seed=14)
    imgs, starts = _queries(base, 3, 2), _starts(3, 3, 6, seed=17)
    points = sum(SIZES)
    assert po.rooms_images_chain_pays(points, 6)
    monkeypatch.setattr(po, "ROOMS_IMAGES_POINT_POSES", points * 6 - 1)
    assert not po.rooms_images_chain_pays(points, 6)
    chains = []
    real = po._rooms_images_chain
    monkeypatch.setattr(po, "_rooms_images_chain", lambda imgs, *a, **k: chains.append(len(imgs)) or real(imgs, *a, **k))
    for rooms in (base, _per_image_colours(base, 3, seed=9)):
        _compare(imgs, rooms, starts, _cfg())
    assert chains == []                                # every image went through omniloc_batch_rooms
    monkeypatch.setattr(po, "ROOMS_IMAGES_POINT_POSES", points * 6)
    _compare(imgs, base, starts, _cfg())
    assert chains == [3]


def test_depth_mask_falls_back_to_one_call_per_room():
    from piccolo_amd import omniloc as po
    base = _rooms((30_000, 60_000), seed=2)
    imgs = _queries(base, 2, 1)
    cfg = _cfg(num_iter=10, depth_mask=True)
    for rooms in (base, _per_image_colours(base, 2, seed=1)):
        starts = _starts(2, 2, 6, seed=4)
        tr_m = [[s[0].clone() for s in row] for row in starts]
        ro_m = [[s[1].clone() for s in row] for row in starts]
        got = po.omniloc_batch_rooms_images(imgs, rooms, tr_m, ro_m, cfg)
        for r, (xyz, rgb) in enumerate(rooms):
            tr, ro = [s[0].clone() for s in starts[r]], [s[1].clone() for s in starts[r]]
            want = po.omniloc_batch_images(imgs, xyz, rgb, tr, ro, cfg)
            for i in range(2):
                for k in range(3):
                    assert torch.equal(got[r][i][k], want[i][k]), (r, i, k)
                assert torch.equal(tr_m[r][i], tr[i]) and torch.equal(ro_m[r][i], ro[i]), (r, i)


@pytest.mark.parametrize("sharpen", [True, False])
def test_localize_images_in_rooms_equals_localize_in_rooms_per_image(sharpen):
    from piccolo_amd import localize, synth
    rooms = _rooms((100_000, 100_000, 100_000), seed=30)
    cfg = Cfg(dataset="Stanford2D-3D-S", sharpen_color=sharpen, **INIT)
    init = localize.get_init_dict(cfg)
    queries = [_query(rooms, r, 40 + r) for r in (2, 0, 1)]
    imgs = [q[0] for q in queries]
    got = localize.localize_images_in_rooms(imgs, imgs, rooms, cfg, init)
    assert len(got) == 3
    for i, (img, t_gt, ypr_gt) in enumerate(queries):
        k, t, R, loss, losses = localize.localize_in_rooms(img, img, rooms, cfg, init)
        assert got[i][0] == k == (2, 0, 1)[i], (i, got[i][0], k)
        assert torch.equal(got[i][1], t) and torch.equal(got[i][2], R) and torch.equal(got[i][3], loss) and torch.equal(got[i][4], losses), i
        t_err, r_err = localize.pose_errors(t, R, t_gt, synth.rot_from_ypr_np(ypr_gt))
        assert localize.stanford_success(t_err, r_err), (i, t_err, r_err)


TIME_COLUMN = 15                                 # t (3), R (9), loss, t_err, r_err, seconds


def test_stanford_harness_groups_images_and_writes_the_same_table(tmp_path, monkeypatch):
    from piccolo_amd import localize
    from test_dataset_harness import _csv_without_time
    root = tmp_path / "stanford"
    files = _write_rooms_tree(root)
    tables, founds, rows = {}, {}, {}
    calls = {"group": [], "single": 0}
    real_group, real_single = localize.localize_images_in_rooms, localize.localize_in_rooms
    monkeypatch.setattr(localize, "localize_images_in_rooms", lambda imgs, *a, **k: calls["group"].append(len(imgs)) or real_group(imgs, *a, **k))

    def counted_single(*a, **k):
        calls["single"] += 1
        return real_single(*a, **k)
    monkeypatch.setattr(localize, "localize_in_rooms", counted_single)
    for n in (1, 4):
        log = tmp_path / ("log%d" % n)
        cfg = Cfg(dataset="Stanford2D-3D-S", area=2, sharpen_color=True, room_search=True, room_search_images=n, **INIT)
        tables[n] = localize.localize_stanford(cfg, None, str(log), root=str(root)).cpu().numpy()
        founds[n] = dict(localize.LAST_RUN["found_rooms"])
        assert localize.LAST_RUN["room_accuracy"] == 1.0
        rows[n] = _csv_without_time(log / "stanford_results.csv")
        assert (log / "results/area_2" / files[0][0]).exists()
    assert calls == {"group": [3], "single": 3}, calls       # N = 1: one image per call; N = 4: the area's three images in ONE call
    assert tables[1].shape == tables[4].shape == (3, 16)
    keep = [c for c in range(16) if c != TIME_COLUMN]
    assert np.array_equal(tables[1][:, keep], tables[4][:, keep], equal_nan=True)
    assert founds[1] == founds[4] and len(founds[4]) == 3
    assert rows[1] == rows[4] and {r[1]: r[-1] for r in rows[4][1:]} == dict(files)


def test_stanford_harness_grouping_skips_out_of_room_images(tmp_path, monkeypatch):
    """an image whose ground truth lies outside its room is skipped (a NaN row) and leaves the groups of the others as they are"""
    import json
    from piccolo_amd import localize
    root = tmp_path / "stanford"
    files = _write_rooms_tree(root)
    pose = root / "pose/area_2" / files[1][0].replace("_rgb.png", "_pose.json")
    d = json.loads(pose.read_text())
    d["camera_location"] = [v + 50.0 for v in d["camera_location"]]
    pose.write_text(json.dumps(d))
    tables, groups = {}, []
    real_group = localize.localize_images_in_rooms
    monkeypatch.setattr(localize, "localize_images_in_rooms", lambda imgs, *a, **k: groups.append(len(imgs)) or real_group(imgs, *a, **k))
    for n in (1, 4):
        cfg = Cfg(dataset="Stanford2D-3D-S", area=2, sharpen_color=True, room_search=True, room_search_images=n, **INIT)
        tables[n] = localize.localize_stanford(cfg, None, None, root=str(root)).cpu().numpy()
        assert len(localize.LAST_RUN["skipped"]) == 1 and len(localize.LAST_RUN["found_rooms"]) == 2
    keep = [c for c in range(16) if c != TIME_COLUMN]
    assert groups == [2], groups                       # the skipped image between them does not split the group
    assert np.isnan(tables[4]).all(axis=1).sum() == 1
    assert np.array_equal(tables[1][:, keep], tables[4][:, keep], equal_nan=True)


def test_room_search_images_on_two_ranks_writes_the_single_process_table(tmp_path):
    from test_dataset_harness import _csv_without_time, _run_main
    files = _write_rooms_tree(tmp_path / "data" / "stanford")
    out = {}
    for n in (1, 4):
        ini = tmp_path / ("rooms%d.ini" % n)
        keys = dict(INIT, dataset="Stanford2D-3D-S", area=2, sharpen_color=True, room_search=True, room_search_images=n)
        ini.write_text("[All]\n" + "".join("%s = %s\n" % kv for kv in keys.items()))
        out[n] = ini
    one = _run_main(["--config", str(out[1])], 1, tmp_path / "r1", cwd=tmp_path)
    two = _run_main(["--config", str(out[4])], 2, tmp_path / "r2", cwd=tmp_path)
    a, b = _csv_without_time(tmp_path / "r1" / "stanford_results.csv"), _csv_without_time(tmp_path / "r2" / "stanford_results.csv")
    assert len(a) == 4 and a == b, (a, b)
    assert a[0][-1] == "found_room" and {r[1]: r[-1] for r in a[1:]} == dict(files)
    for o in (one, two):
        assert o.count("Room accuracy : 1.0") == 1, o[-2000:]
