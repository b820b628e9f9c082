"""GPU tests of the pose information and the Levenberg-Marquardt polish for all (room, image) winners of a rooms x images chain:
pcl_pose_information_rooms, pcl_gn_refine_rooms, the ops wrappers, omniloc_batch_rooms_images_polished and the harness key
room_search_polish.  Build-defined: the reference has none of them.  Every assertion but one is BIT equality against the single-room
calls that test_pose_information.py and test_gn_refine.py pin to the float64 models; the one number that is not the single call's — the
loss of a polished entry, S1 / M of the polish's own record — is compared bit for bit with that record.

Rooms of 300 / 1025 / 6,000 / 20,000 points (room_helpers, side by side) are 1 / 2 / 6 / 20 chunks of the per-point pass: one step only
(below PCL_INFO_MIN_STEPS), a chunk remainder with a one-point tail, and rooms of different chunk counts side by side — a wrong block
decode or row offset lands in another room's rows.  3 images (no power of two), quantised k / 255, 64 x 128."""
import os

import numpy as np
import pytest
import torch

from room_helpers import image_starts, per_image_colours, query, rooms as make_rooms

pytestmark = pytest.mark.gpu

SIZES = (300, 1025, 6_000, 20_000)
RES = (64, 128)
I = 3
FMTS = ("u8", "f16", "f32")
GN_FIELDS = ("trans", "rot", "sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats", "cov")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


_SCENES = {}


def scene(ops, sizes=SIZES, nimages=I, seed=0):
    """-> dict: rooms (xyz, rgb), cols[r][i] per-image colours, imgs (image i shows room i mod R), shared / sets / single clouds in ONE
    packed order per room, and one start pose per (room, image), row r * I + i"""
    key = (sizes, nimages, seed)
    if key not in _SCENES:
        base = make_rooms(sizes, seed)
        R = len(base)
        cols = [c for _, c in per_image_colours(base, nimages, seed=seed + 1)]
        imgs = [query(base, i % R, seed + 5 + i, res=RES)[0] for i in range(nimages)]
        shared = [ops.Cloud(x, c) for x, c in base]
        sets = [ops.Cloud.with_color_sets(x, cols[r], order=shared[r].order) for r, (x, _) in enumerate(base)]
        single = [[ops.Cloud(x, cols[r][i], order=shared[r].order) for i in range(nimages)] for r, (x, _) in enumerate(base)]
        st = image_starts(R, nimages, 2, seed=seed + 3)
        trans = torch.stack([st[r][i][0][1] for r in range(R) for i in range(nimages)]).contiguous()
        rot = torch.stack([st[r][i][1][1] for r in range(R) for i in range(nimages)]).contiguous()
        _SCENES[key] = dict(base=base, cols=cols, imgs=imgs, shared=shared, sets=sets, single=single, trans=trans, rot=rot, R=R, I=nimages)
    return _SCENES[key]


def clouds_of(s, colours):
    """(the call's room clouds, alone[r][i]: the cloud of the single call of (r, i))"""
    if colours == "shared":
        return s["shared"], [[s["shared"][r]] * s["I"] for r in range(s["R"])]
    return s["sets"], s["single"]


def winners_of(trans, rot):
    win = torch.full((trans.shape[0], 16), float("nan"), device="cuda")
    win[:, 0:3], win[:, 13:16] = trans, rot
    return win


# ------------------------------------------------------------------------------------------------ 1. the information rows

@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("fmt", FMTS)
def test_information_rows_are_the_single_room_calls(ops, fmt, colours):
    """row r * I + i of (H, b, stats, cov) == ops.pose_information of that pose against room r's cloud, colour set i and panorama i alone;
    pose strides 3 and 16; rows of two rooms differ, rows of two images differ"""
    s = scene(ops)
    R = s["R"]
    clouds, alone = clouds_of(s, colours)
    panos = [ops.Pano(im, fmt=fmt) for im in s["imgs"]]
    trans, rot = s["trans"], s["rot"]
    rows = ops.pose_information_rooms(clouds, panos, trans, rot)
    rows16 = ops.pose_information_rooms_at_winners(clouds, panos, winners_of(trans, rot))
    assert all(same_bits(a, b) for a, b in zip(rows, rows16))
    assert rows[0].shape == (R * I, 6, 6) and rows[1].shape == (R * I, 6) and rows[2].shape == (R * I, 5) and rows[3].shape == (R * I, 6, 6)
    for r in range(R):
        for i in range(I):
            p = r * I + i
            want = ops.pose_information(alone[r][i], panos[i], trans[p:p + 1], rot[p:p + 1])
            for got, w, what in zip(rows, want, ("H", "b", "stats", "cov")):
                assert same_bits(got[p:p + 1], w), (fmt, colours, r, i, what)
    assert (rows[2][:, 0] > 0).all()                                                        # every pose keeps points
    assert not same_bits(rows[0][0 * I + 1], rows[0][2 * I + 1]) and not same_bits(rows[0][3 * I + 0], rows[0][3 * I + 1])


# ------------------------------------------------------------------------------------------------ 2. the polish

@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("fmt", FMTS)
def test_polish_rows_are_the_single_room_calls(ops, fmt, colours):
    """iters = 4 with the trace: every field and the trace of (r, i) == ops.gauss_newton_refine alone; a pose that is not finite in a middle
    room (status 1, one evaluation, NaN cov: its blocks return before their point loop) moves no other pose's bits"""
    s = scene(ops)
    R = s["R"]
    clouds, alone = clouds_of(s, colours)
    panos = [ops.Pano(im, fmt=fmt) for im in s["imgs"]]
    bad = 2 * I + 1
    trans, rot = s["trans"].clone(), s["rot"]
    trans[bad, 1] = float("nan")
    res = ops.gauss_newton_refine_rooms(clouds, panos, trans, rot, iters=4, trace=True)
    res16 = ops.gauss_newton_refine_rooms_at_winners(clouds, panos, winners_of(trans, rot), iters=4, trace=True)
    assert res["trace"].shape == (5, R * I, 16)
    for r in range(R):
        for i in range(I):
            p = r * I + i
            want = ops.gauss_newton_refine(alone[r][i], panos[i], trans[p:p + 1], rot[p:p + 1], iters=4, trace=True)
            for key in GN_FIELDS:
                assert same_bits(res[key][p:p + 1], want[key]), (fmt, colours, r, i, key)
                assert same_bits(res16[key][p:p + 1], want[key]), (fmt, colours, r, i, key)
            assert same_bits(res["trace"][:, p:p + 1], want["trace"]) and same_bits(res16["trace"][:, p:p + 1], want["trace"]), (r, i)
    status, evals = res["status"].tolist(), res["evaluations"].tolist()
    assert status[bad] == 1 and evals[bad] == 1 and (res["trace"][1:, bad] == 0).all() and torch.isnan(res["cov"][bad]).all()
    assert max(evals) == 5 and float(res["accepted"].max()) > 1
    # the information call at that pose: the single call's record, the sign bits of its NaNs included
    info = ops.pose_information_rooms(clouds, panos, trans, rot)
    for got, w in zip(info, ops.pose_information(alone[2][1], panos[1], trans[bad:bad + 1], rot[bad:bad + 1])):
        assert same_bits(got[bad:bad + 1], w)
    assert float(info[2][bad, 4]) == 1 and torch.isnan(info[3][bad]).all()
    # the same call without the frozen pose: every other row keeps its bits
    res2 = ops.gauss_newton_refine_rooms(clouds, panos, s["trans"], rot, iters=4, trace=True)
    keep = [p for p in range(R * I) if p != bad]
    assert all(same_bits(res[key][keep], res2[key][keep]) for key in GN_FIELDS) and same_bits(res["trace"][:, keep], res2["trace"][:, keep])
    assert float(res2["status"][bad]) != 1


# ------------------------------------------------------------------------------------------------ 3. one room, one image

@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_one_room_is_the_images_call_and_one_image_the_single_calls(ops, colours):
    s = scene(ops)
    R = s["R"]
    clouds, alone = clouds_of(s, colours)
    panos = [ops.Pano(im, fmt="f16") for im in s["imgs"]]
    trans, rot = s["trans"], s["rot"]
    for r in (0, 3):
        sl = slice(r * I, (r + 1) * I)
        one = ops.gauss_newton_refine_rooms(clouds[r:r + 1], panos, trans[sl], rot[sl], iters=4, trace=True)
        img = ops.gauss_newton_refine_images(clouds[r], panos, trans[sl], rot[sl], iters=4, trace=True)
        assert all(same_bits(one[key], img[key]) for key in GN_FIELDS + ("trace",)), r
        a, b = ops.pose_information_rooms(clouds[r:r + 1], panos, trans[sl], rot[sl]), ops.pose_information_images(clouds[r], panos, trans[sl], rot[sl])
        assert all(same_bits(x, y) for x, y in zip(a, b)), r
    if colours == "shared":                                   # (one image: one colour set per room)
        i = 1
        idx = [r * I + i for r in range(R)]
        res = ops.gauss_newton_refine_rooms(clouds, panos[i:i + 1], trans[idx], rot[idx], iters=4, trace=True)
        info = ops.pose_information_rooms(clouds, panos[i:i + 1], trans[idx], rot[idx])
        for r in range(R):
            p = idx[r]
            want = ops.gauss_newton_refine(alone[r][i], panos[i], trans[p:p + 1], rot[p:p + 1], iters=4, trace=True)
            assert all(same_bits(res[key][r:r + 1], want[key]) for key in GN_FIELDS) and same_bits(res["trace"][:, r:r + 1], want["trace"]), r
            for got, w in zip(info, ops.pose_information(alone[r][i], panos[i], trans[p:p + 1], rot[p:p + 1])):
                assert same_bits(got[r:r + 1], w), r


# ------------------------------------------------------------------------------------------------ 4. more images than one launch names

def test_sixty_six_images_run_in_two_groups(ops):
    """two rooms (300, 1025) x 66 images, a colour set per image, iters = 1: rows 0, 63, 64 and 65 of both rooms == their single calls —
    two pass launches per evaluation, colour sets and partial rows counted from the call's first image"""
    n_img, keep = 66, (0, 63, 64, 65)
    base = make_rooms(SIZES[:2], 2)
    imgs = [query(base, i % 2, 20 + i, res=RES)[0] for i in range(3)]
    p3 = [ops.Pano(im, fmt="u8") for im in imgs]
    panos = [p3[k % 3] for k in range(n_img)]
    rng = np.random.default_rng(5)
    st = image_starts(2, 1, 4, seed=9)
    clouds, single, trans, rot = [], [], [], []
    for r, (x, c) in enumerate(base):
        cols = [torch.roll(c, k, 0).contiguous() for k in range(n_img)]
        first = ops.Cloud(x, cols[0])
        clouds.append(ops.Cloud.with_color_sets(x, cols, order=first.order))
        single.append({i: ops.Cloud(x, cols[i], order=first.order) for i in keep})
        for k in range(n_img):
            trans.append(st[r][0][0][k % 4] + torch.from_numpy(0.01 * rng.random(3).astype(np.float32)).cuda())
            rot.append(st[r][0][1][k % 4])
    trans, rot = torch.stack(trans).contiguous(), torch.stack(rot).contiguous()
    res = ops.gauss_newton_refine_rooms(clouds, panos, trans, rot, iters=1, trace=True)
    info = ops.pose_information_rooms(clouds, panos, trans, rot)
    assert res["trace"].shape == (2, 2 * n_img, 16)
    for r in range(2):
        for i in keep:
            p = r * n_img + i
            want = ops.gauss_newton_refine(single[r][i], panos[i], trans[p:p + 1], rot[p:p + 1], iters=1, trace=True)
            for key in GN_FIELDS:
                assert same_bits(res[key][p:p + 1], want[key]), (r, i, key)
            assert same_bits(res["trace"][:, p:p + 1], want["trace"]), (r, i)
            for got, w in zip(info, ops.pose_information(single[r][i], panos[i], trans[p:p + 1], rot[p:p + 1])):
                assert same_bits(got[p:p + 1], w), (r, i)
    assert not same_bits(res["H"][0], res["H"][64]) and not same_bits(res["H"][64], res["H"][n_img + 64])


# ------------------------------------------------------------------------------------------------ 5. at the winners of the rooms x images chain

@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_polish_at_the_winners_of_the_rooms_images_chain(ops, colours, pruned):
    """a rooms x images engine of 4 candidates per (room, image) run for 12 iterations — plain, or pruned to 2 after 4 —, then ONE polish
    of all winners: row (r, i) == gauss_newton_refine_at_winners of that room, colour set and image alone"""
    s = scene(ops)
    R = s["R"]
    clouds, alone = clouds_of(s, colours)
    panos = [ops.Pano(im, fmt="f16") for im in s["imgs"]]
    st = image_starts(R, I, 4, seed=17)
    tr = torch.cat([st[r][i][0] for r in range(R) for i in range(I)])
    ro = torch.cat([st[r][i][1] for r in range(R) for i in range(I)])
    boxes = [ops.quantile_box(x, 0.05) for x, _ in s["base"]]
    gd = ops.GradientDescentRoomsImages(list(zip(clouds, boxes)), panos, tr, ro, lr=0.1, patience=5, factor=0.8)
    if pruned:
        gd.run(4)
        gd, _ = gd.pruned(2)
        gd.run(8)
    else:
        gd.run(12)
    wins = gd.winner()
    assert wins.shape == (R * I, 16)
    res = ops.gauss_newton_refine_rooms_at_winners(clouds, panos, wins, iters=4)
    cov = ops.pose_information_rooms_at_winners(clouds, panos, wins)[3]
    for r in range(R):
        for i in range(I):
            p = r * I + i
            w1 = wins[p:p + 1].contiguous()
            want = ops.gauss_newton_refine_at_winners(alone[r][i], panos[i], w1, iters=4)
            for key in GN_FIELDS:
                assert same_bits(res[key][p:p + 1], want[key]), (colours, pruned, r, i, key)
            assert same_bits(cov[p:p + 1], ops.pose_information_at_winners(alone[r][i], panos[i], w1)[3]), (r, i)


# ------------------------------------------------------------------------------------------------ 6. the surface

BASE = dict(num_iter=12, num_input=6, lr=0.1, patience=5, factor=0.9, out_of_room_quantile=0.05)


@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_the_surface(ops, colours):
    """omniloc_batch_rooms_images_polished entry (r, i) against omniloc_batch(imgs[i], xyz_r, rgb_r[i], ...) under the same cfg: t, R and cov
    bit for bit; the loss == float32(S1) / float32(M) of the polish's record where it took a step, the chain's own where it did not (both
    occur); the written-back leaves and chain_loss are omniloc_batch_rooms_images'; with pose_covariance alone the first three entries
    are the plain call's"""
    from conftest import Cfg
    from piccolo_amd import omniloc as po
    s = scene(ops)
    R, ims = s["R"], s["imgs"]
    rooms = [(x, s["cols"][r] if colours == "sets" else c) for r, (x, c) in enumerate(s["base"])]
    rgb_of = lambda r, i: rooms[r][1][i] if colours == "sets" else rooms[r][1]      # noqa: E731
    st = image_starts(R, I, 6, seed=21)

    def starts():
        return [[st[r][i][0].clone() for i in range(I)] for r in range(R)], [[st[r][i][1].clone() for i in range(I)] for r in range(R)]

    def leaves(tl, rl):
        return [t.cpu() for ts in tl for t in ts], [r.cpu() for rs in rl for r in rs]

    tl, rl = starts()
    base = po.omniloc_batch_rooms_images(ims, rooms, tl, rl, Cfg(**BASE))
    base_t, base_r = leaves(tl, rl)
    base_loss = torch.stack([torch.stack([base[r][i][2].reshape(()) for i in range(I)]) for r in range(R)])
    clouds = [po.packed_cloud_sets(x, c) if colours == "sets" else po.packed_cloud(x, c) for x, c in rooms]
    panos = po._chain_panos(ims, max(int(x.shape[0]) for x, _ in rooms))
    seen = set()
    for kw in (dict(gn_iters=3), dict(gn_iters=3, pose_covariance=True), dict(gn_iters=1, gn_step_cap=1e-30, pose_covariance=True)):
        cfg = Cfg(**BASE, **kw)
        tl, rl = starts()
        got, chain_loss = po.omniloc_batch_rooms_images_polished(ims, rooms, tl, rl, cfg)
        got_t, got_r = leaves(tl, rl)
        assert all(same_bits(a, b) for a, b in zip(got_t + got_r, base_t + base_r))          # the written-back leaves stay the chain's
        assert chain_loss.shape == (R, I) and chain_loss.device.type == "cpu" and same_bits(chain_loss, base_loss)
        # the record of the polish at the chain's winners, from the pieces
        tl, rl = starts()
        gd = po._chain("gd_rooms_images", ims, rooms, torch.cat([t for ts in tl for t in ts]), torch.cat([r for rs in rl for r in rs]), cfg, True)
        gn = po.gn_schedule(cfg)
        res = ops.gauss_newton_refine_rooms_at_winners(clouds, panos, gd.winners(R * I), iters=gn[0], **gn[1])
        acc, status, stats = res["accepted"].cpu().numpy(), res["status"].cpu().numpy(), res["stats"].cpu().numpy()
        took = (acc > 1) & ((status == 0) | (status == 3))
        for r in range(R):
            for i in range(I):
                p, g = r * I + i, got[r][i]
                one = po.omniloc_batch(ims[i], rooms[r][0], rgb_of(r, i), st[r][i][0].clone(), st[r][i][1].clone(), cfg, {})
                assert len(g) == len(one) == (4 if "pose_covariance" in kw else 3)
                assert g[0].shape == (3, 1) and g[1].shape == (3, 3) and g[2].shape == ()
                assert same_bits(g[0], one[0]) and same_bits(g[1], one[1]), (colours, kw, r, i)
                if "pose_covariance" in kw:
                    assert g[3].shape == (6, 6) and same_bits(g[3], one[3]), (colours, kw, r, i)
                if took[p]:
                    want = np.float32(stats[p, 1]) / np.float32(stats[p, 0])
                    assert np.float32(g[2].item()).tobytes() == np.float32(want).tobytes(), (colours, kw, r, i)
                    assert not same_bits(g[0], base[r][i][0])
                else:
                    assert all(same_bits(a, b) for a, b in zip(g[:3], base[r][i])) and same_bits(g[2], one[2]), (colours, kw, r, i)
                seen.add(bool(took[p]))
    assert seen == {True, False}
    # pose_covariance alone: the plain call's three entries, and the single call's covariance
    tl, rl = starts()
    got, chain_loss = po.omniloc_batch_rooms_images_polished(ims, rooms, tl, rl, Cfg(**BASE, pose_covariance=True))
    assert same_bits(chain_loss, base_loss)
    for r in range(R):
        for i in range(I):
            one = po.omniloc_batch(ims[i], rooms[r][0], rgb_of(r, i), st[r][i][0].clone(), st[r][i][1].clone(), Cfg(**BASE, pose_covariance=True), {})
            assert len(got[r][i]) == 4 and all(same_bits(a, b) for a, b in zip(got[r][i][:3], base[r][i]))
            assert same_bits(got[r][i][3], one[3]), (r, i)
    # one image: the one-image rooms chain, polished
    tl, rl = starts()
    first, loss1 = po.omniloc_batch_rooms_images_polished(ims[:1], [(x, rgb_of(r, 0)) for r, (x, _) in enumerate(rooms)], [t[:1] for t in tl],
                                                          [r[:1] for r in rl], Cfg(**BASE, gn_iters=3, pose_covariance=True))
    assert loss1.shape == (R, 1) and same_bits(loss1[:, 0], base_loss[:, 0])
    for r in range(R):
        one = po.omniloc_batch(ims[0], rooms[r][0], rgb_of(r, 0), st[r][0][0].clone(), st[r][0][1].clone(), Cfg(**BASE, gn_iters=3, pose_covariance=True), {})
        assert same_bits(first[r][0][0], one[0]) and same_bits(first[r][0][1], one[1]) and same_bits(first[r][0][3], one[3]), r


# ------------------------------------------------------------------------------------------------ 7. localize_images_in_rooms

INIT = dict(num_trans=30, xy_only=False, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4, criterion="loss_histogram", num_intermediate=20,
            num_input=8, num_split_h=4, num_split_w=4, lr=0.1, num_iter=30, patience=5, factor=0.8, out_of_room_quantile=0.05, sample_rate=1,
            parallel=True, num_bins=256)
POLISH = dict(room_search=True, room_search_polish=True, gn_iters=3, pose_covariance=True)


@pytest.mark.parametrize("sharpen", [False, True])
def test_localize_images_in_rooms_with_the_key(monkeypatch, sharpen):
    """found room and every room's loss == the plain run's; entry i == localize_in_rooms of image i; pose, loss and cov are the found room's
    polished entry"""
    from conftest import Cfg
    from piccolo_amd import localize
    rooms = make_rooms((20_000, 30_000, 25_000), seed=30)
    imgs = [query(rooms, r, 40 + r)[0] for r in (2, 0, 1)]
    plain_cfg = Cfg(dataset="Stanford2D-3D-S", sharpen_color=sharpen, **INIT)
    cfg = Cfg(dataset="Stanford2D-3D-S", sharpen_color=sharpen, **INIT, **POLISH)
    init = localize.get_init_dict(cfg)
    plain = localize.localize_images_in_rooms(imgs, imgs, rooms, plain_cfg, init)
    calls = []
    inner = localize.omniloc_batch_rooms_images_polished
    monkeypatch.setattr(localize, "omniloc_batch_rooms_images_polished", lambda *a, **k: calls.append(inner(*a, **k)) or calls[-1])
    got = localize.localize_images_in_rooms(imgs, imgs, rooms, cfg, init)
    assert len(calls) == 1 and len(got) == 3
    entries, chain_loss = calls[0]
    for i in range(3):
        k = got[i][0]
        assert len(got[i]) == 6 and k == plain[i][0] and same_bits(got[i][4], plain[i][4]), i
        assert same_bits(got[i][4], chain_loss[:, i]) and k == int(torch.argmin(chain_loss[:, i]))
        for a, b in zip(got[i][1:4] + got[i][5:6], entries[k][i]):
            assert same_bits(a, b), i
        assert got[i][5].shape == (6, 6) and torch.isfinite(got[i][5]).all()
        alone = localize.localize_in_rooms(imgs[i], imgs[i], rooms, cfg, init)
        assert alone[0] == k and len(alone) == 6 and all(same_bits(a, b) for a, b in zip(alone[1:], got[i][1:])), i
    # without pose_covariance the tuples keep their five entries
    no_cov = Cfg(dataset="Stanford2D-3D-S", sharpen_color=sharpen, **INIT, room_search=True, room_search_polish=True, gn_iters=3)
    five = localize.localize_images_in_rooms(imgs, imgs, rooms, no_cov, init)
    assert all(len(f) == 5 and f[0] == g[0] and same_bits(f[1], g[1]) and same_bits(f[4], g[4]) for f, g in zip(five, got))


# ------------------------------------------------------------------------------------------------ 8. the harness

def test_harness_room_search_polish(tmp_path):
    """room_search_images = 1 and 3 write the same CSV rows; the header ends found_room, sigma_t (m), sigma_r (degrees) with finite positive
    sigmas; found_room and room_accuracy are those of the run without the polish keys"""
    import csv
    from conftest import Cfg
    from piccolo_amd import localize
    from test_dataset_harness import _csv_without_time
    from test_room_search import _write_rooms_tree
    root = tmp_path / "stanford"
    _write_rooms_tree(root)
    keys = dict(INIT, dataset="Stanford2D-3D-S", area=2, sharpen_color=True, room_search=True)
    log = tmp_path / "plain"
    localize.localize_stanford(Cfg(**keys, room_search_images=3), None, str(log), root=str(root))
    plain_acc, plain_found = localize.LAST_RUN["room_accuracy"], dict(localize.LAST_RUN["found_rooms"])
    rows = {}
    for n in (1, 3):
        log = tmp_path / ("log%d" % n)
        cfg = Cfg(**keys, room_search_images=n, room_search_polish=True, gn_iters=3, pose_covariance=True)
        table = localize.localize_stanford(cfg, None, str(log), root=str(root)).cpu().numpy()
        assert table.shape == (3, 16) and not np.isnan(table).any()
        assert localize.LAST_RUN["room_accuracy"] == plain_acc and localize.LAST_RUN["found_rooms"] == plain_found
        rows[n] = _csv_without_time(log / "stanford_results.csv")
    assert rows[1] == rows[3] and len(rows[1]) == 4
    with open(tmp_path / "log3" / "stanford_results.csv") as f:
        full = list(csv.reader(f))
    assert full[0][-3:] == ["found_room", "sigma_t (m)", "sigma_r (degrees)"] and full[0][:-3] == localize.STANFORD_HEADER
    for r in full[1:]:
        assert len(r) == len(full[0]) and all(np.isfinite(float(v)) and float(v) > 0 for v in r[-2:])
        assert r[-3] == {os.path.basename(f): name for f, name in plain_found.items()}[r[1]]
