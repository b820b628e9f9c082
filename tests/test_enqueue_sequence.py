"""GPU tests of the host protocol of the GD front end: the SEQUENCE of C entry points every public refinement path enqueues, call by call.

Every enqueuing C call of piccolo_amd/ops.py reports its entry point's name to _lib.check; the tests record those names while a path runs
twice from empty caches — the second call meets the packed clouds and panoramas, the cached engine and its captured graph — and compare
both sequences with literal lists.  The lists were recorded on the MI355X from the commit BEFORE the front end's drivers were merged into
one (omniloc._drive), so they pin what that refactor, and whatever changes next how a chain is acquired and run, must keep: no
pcl_gd_set_pano_groups launch that appears or disappears, no added pcl_gd_init*, no chain that turns eager or replayed.

Shapes are the smallest that reach every branch (the host protocol is under test, not the kernels): two rooms of about 2,500 points on a
32 x 64 panorama, 2 images, 4 candidates per group, num_iter 4.

LADDERS are the paths through the layer above the driver: the polished forms and every fallback of the images and rooms entry points (a
fallback is forced by patching a Python constant, never the library).  Their lists, and tests/golden/front_end_ladders.npz — every tensor
such a path returns and writes back, `python tests/test_enqueue_sequence.py OUT.npz` —, were recorded on the MI355X from the commit BEFORE
those entry points were given one images ladder and one rooms ladder."""
import pytest
import torch

from conftest import Cfg, load_golden

pytestmark = pytest.mark.gpu

H, W = 32, 64
SIZES = (2500, 2399)
R, I, B = 2, 2, 4
PRUNE = dict(prune_iters=2, prune_keep=2)
ROBUST = dict(robust_iters=[2])


def _cfg(**kw):
    base = dict(lr=0.1, num_iter=4, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=B)
    base.update(kw)
    return Cfg(**base)


_SCENE = {}


def scene():
    """rooms (shared colours), rooms_c (a colour list per room), imgs, starts[r][i] = (trans, rot): built once, never written to"""
    if not _SCENE:
        import room_helpers as rh
        rooms = rh.rooms(SIZES)
        _SCENE.update(rooms=rooms, rooms_c=rh.per_image_colours(rooms, I), imgs=[rh.query(rooms, i, 5 + i, (H, W))[0] for i in range(I)],
                      starts=rh.image_starts(R, I, B))
    return _SCENE


def _tr(s, r=0, i=0):
    return s["starts"][r][i][0].clone()


def _ro(s, r=0, i=0):
    return s["starts"][r][i][1].clone()


def _one(po, s, **kw):
    xyz, rgb = s["rooms"][0]
    return po.omniloc_batch(s["imgs"][0], xyz, rgb, _tr(s), _ro(s), _cfg(**kw), {})


def _images(po, s, colours, robust=False, **kw):
    xyz, rgb = s["rooms_c" if colours else "rooms"][0]
    args = (s["imgs"], xyz, rgb, [_tr(s, 0, i) for i in range(I)], [_ro(s, 0, i) for i in range(I)])
    if robust:
        return po.omniloc_batch_images_robust(*args, _cfg(**ROBUST, **kw))
    return po.omniloc_batch_images(*args, _cfg(**kw))


def _rooms_one(po, s, **kw):
    return po.omniloc_batch_rooms(s["imgs"][0], s["rooms"], [_tr(s, r) for r in range(R)], [_ro(s, r) for r in range(R)], _cfg(**kw))


def _rooms_images(po, s, colours, **kw):
    return po.omniloc_batch_rooms_images(s["imgs"], s["rooms_c" if colours else "rooms"], [[_tr(s, r, i) for i in range(I)] for r in range(R)],
                                         [[_ro(s, r, i) for i in range(I)] for r in range(R)], _cfg(**kw))


def _images_form(po, s, form, colours, n=I, batch_mode=None, **kw):
    """omniloc_batch_images + form ("", "_robust", "_polished") over the first n images -> (what it returns, the written-back leaves)"""
    xyz, rgb = s["rooms_c" if colours else "rooms"][0]
    tr, ro = [_tr(s, 0, i) for i in range(n)], [_ro(s, 0, i) for i in range(n)]
    out = getattr(po, "omniloc_batch_images" + form)(s["imgs"][:n], xyz, rgb[:n] if colours else rgb, tr, ro, _cfg(**kw),
                                                     **({} if batch_mode is None else {"batch_mode": batch_mode}))
    return out, tr + ro


def _rooms_form(po, s, form, colours, n=I, **kw):
    """omniloc_batch_rooms_images + form ("", "_polished") over the first n images -> (what it returns, the written-back leaves)"""
    rooms = [(xyz, rgb[:n]) for xyz, rgb in s["rooms_c"]] if colours else s["rooms"]
    tr, ro = [[_tr(s, r, i) for i in range(n)] for r in range(R)], [[_ro(s, r, i) for i in range(n)] for r in range(R)]
    out = getattr(po, "omniloc_batch_rooms_images" + form)(s["imgs"][:n], rooms, tr, ro, _cfg(**kw))
    return out, sum(tr, []) + sum(ro, [])


def _rooms_one_form(po, s, **kw):
    tr, ro = [_tr(s, r) for r in range(R)], [_ro(s, r) for r in range(R)]
    return po.omniloc_batch_rooms(s["imgs"][0], s["rooms"], tr, ro, _cfg(**kw)), tr + ro


GN, COV = dict(gn_iters=1), dict(pose_covariance=True)

# how a fallback is forced (tests/test_room_images.py's way): FORCED[key](monkeypatch, po, ops, scene), for the paths of LADDERS named "<key>:..."
FORCED = {
    "per_image": lambda m, po, ops, s: m.setattr(po, "ROOMS_IMAGES_POINT_POSES", sum(int(xyz.shape[0]) for xyz, _ in s["rooms"]) * B - 1),
    "one_set": lambda m, po, ops, s: m.setattr(ops, "max_color_sets", lambda n: 1),
    "per_room": lambda m, po, ops, s: m.setattr(po, "DEPTH_SHARED_ROOM_CANDIDATES", I * B - 1),
    "room_cap": lambda m, po, ops, s: m.setattr(ops._lib, "GD_MAX_ROOMS", 1),
}

LADDERS = {
    "polished_shared_gn": lambda po, s: _images_form(po, s, "_polished", False, **GN),
    "polished_shared_cov": lambda po, s: _images_form(po, s, "_polished", False, **COV),
    "polished_list_gn_cov": lambda po, s: _images_form(po, s, "_polished", True, **GN, **COV),
    "polished_robust_gn": lambda po, s: _images_form(po, s, "_polished", False, **ROBUST, **GN),
    "polished_prune_gn": lambda po, s: _images_form(po, s, "_polished", False, **PRUNE, **GN),
    "polished_eager_gn": lambda po, s: _images_form(po, s, "_polished", False, gd_graph=False, **GN),
    "polished_one_image": lambda po, s: _images_form(po, s, "_polished", False, n=1, **GN),
    "images_robust_one_image": lambda po, s: _images_form(po, s, "_robust", False, n=1, **ROBUST),
    "images_sequential": lambda po, s: _images_form(po, s, "", False, batch_mode=False),
    "rooms_polished_shared_gn_cov": lambda po, s: _rooms_form(po, s, "_polished", False, **GN, **COV),
    "rooms_polished_list_gn": lambda po, s: _rooms_form(po, s, "_polished", True, **GN),
    "rooms_polished_prune_cov": lambda po, s: _rooms_form(po, s, "_polished", False, **PRUNE, **COV),
    "rooms_polished_one_image": lambda po, s: _rooms_form(po, s, "_polished", False, n=1, **GN),
    "per_image:rooms_images_shared": lambda po, s: _rooms_form(po, s, "", False),
    "per_image:rooms_images_list": lambda po, s: _rooms_form(po, s, "", True),
    "per_image:rooms_polished": lambda po, s: _rooms_form(po, s, "_polished", False, **GN),
    "one_set:images_list": lambda po, s: _images_form(po, s, "", True),
    "one_set:images_robust_list": lambda po, s: _images_form(po, s, "_robust", True, **ROBUST),
    "one_set:polished_list": lambda po, s: _images_form(po, s, "_polished", True, **GN),
    "one_set:rooms_images_list": lambda po, s: _rooms_form(po, s, "", True),
    "one_set:rooms_polished_list": lambda po, s: _rooms_form(po, s, "_polished", True, **GN),
    "per_room:rooms_images_depth": lambda po, s: _rooms_form(po, s, "", False, depth_mask=True),
    "room_cap:rooms": _rooms_one_form,
    "room_cap:rooms_images": lambda po, s: _rooms_form(po, s, "", False),
    "room_cap:rooms_polished": lambda po, s: _rooms_form(po, s, "_polished", False, **GN),
}

PATHS = {
    "omniloc": lambda po, s: po.omniloc(s["imgs"][0], *s["rooms"][0], _tr(s), _ro(s), 0, _cfg(), {}),
    "omniloc_all": lambda po, s: po.omniloc_all(s["imgs"][0], *s["rooms"][0], _tr(s), _ro(s), _cfg()),
    "batch_eager": lambda po, s: _one(po, s, gd_graph=False),
    "batch_replay": lambda po, s: _one(po, s, gd_graph=True),
    "batch_prune": lambda po, s: _one(po, s, **PRUNE),
    "batch_prune_eager": lambda po, s: _one(po, s, gd_graph=False, **PRUNE),
    "batch_robust": lambda po, s: _one(po, s, **ROBUST),
    "batch_robust_eager": lambda po, s: _one(po, s, gd_graph=False, **ROBUST),
    "batch_cov_gn": lambda po, s: _one(po, s, pose_covariance=True, gn_iters=1),
    "images_shared": lambda po, s: _images(po, s, False),
    "images_shared_eager": lambda po, s: _images(po, s, False, gd_graph=False),
    "images_list": lambda po, s: _images(po, s, True),
    "images_list_prune": lambda po, s: _images(po, s, True, **PRUNE),
    "images_list_depth": lambda po, s: _images(po, s, True, depth_mask=True),
    "images_list_depth_prune": lambda po, s: _images(po, s, True, depth_mask=True, **PRUNE),
    "images_robust": lambda po, s: _images(po, s, False, robust=True),
    "images_robust_list_eager": lambda po, s: _images(po, s, True, robust=True, gd_graph=False),
    "rooms": _rooms_one,
    "rooms_eager": lambda po, s: _rooms_one(po, s, gd_graph=False),
    "rooms_prune": lambda po, s: _rooms_one(po, s, **PRUNE),
    "rooms_prune_eager": lambda po, s: _rooms_one(po, s, gd_graph=False, **PRUNE),
    "rooms_depth": lambda po, s: _rooms_one(po, s, depth_mask=True),
    "rooms_images_shared": lambda po, s: _rooms_images(po, s, False),
    "rooms_images_shared_eager": lambda po, s: _rooms_images(po, s, False, gd_graph=False),
    "rooms_images_list": lambda po, s: _rooms_images(po, s, True),
    "rooms_images_list_prune": lambda po, s: _rooms_images(po, s, True, **PRUNE),
    "rooms_images_depth": lambda po, s: _rooms_images(po, s, False, depth_mask=True),
    "rooms_images_depth_prune": lambda po, s: _rooms_images(po, s, False, depth_mask=True, **PRUNE),
}
PATHS.update(LADDERS)


def _force(m, name, po, s):
    from piccolo_amd import ops
    if ":" in name:
        FORCED[name.split(":")[0]](m, po, ops, s)


def record(monkeypatch, name):
    """-> [the entry points of the first call of PATHS[name] from empty caches, those of the second call]"""
    from piccolo_amd import _lib
    from piccolo_amd import omniloc as po
    _lib.load()
    s, seen, real = scene(), [], _lib.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(_lib, "check", check)
    _force(monkeypatch, name, po, s)
    po._cache.clear()
    out = []
    for _ in range(2):
        del seen[:]
        PATHS[name](po, s)
        out.append(list(seen))
    torch.cuda.synchronize()
    po._cache.clear()
    return out


# recorded on the MI355X from the parent of the commit that introduced omniloc._drive: (first call from empty caches, second call)
EXPECTED = {
    "batch_cov_gn": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss"]),
    "batch_eager": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_run", "pcl_gd_winner"]),
    "batch_prune": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_init", "pcl_gd_prune", "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_winner"]),
    "batch_prune_eager": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_prune", "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_prune", "pcl_gd_run", "pcl_gd_winner"]),
    "batch_replay": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "batch_robust": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_run_weighted", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_winner"]),
    "batch_robust_eager": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_run", "pcl_gd_winner",
         "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_run_weighted", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_run", "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_run_weighted", "pcl_gd_winner"]),
    "images_list": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_gd_init",
         "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "images_list_depth": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_depth_default",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_depth_chain", "pcl_gd_winner"],
        ["pcl_depth_default", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_depth_chain", "pcl_gd_winner"]),
    "images_list_depth_prune": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_depth_default",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_depth_chain", "pcl_gd_prune", "pcl_gd_run_depth_chain", "pcl_gd_winner"],
        ["pcl_depth_default", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_depth_chain", "pcl_gd_prune",
         "pcl_gd_run_depth_chain", "pcl_gd_winner"]),
    "images_list_prune": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_gd_init",
         "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_init", "pcl_gd_prune", "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_winner"]),
    "images_robust": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init_weight_sets",
         "pcl_gd_set_pano_groups", "pcl_gd_run_weight_sets", "pcl_gd_winner", "pcl_point_residuals_images", "pcl_robust_weights_rows",
         "pcl_gd_run_weight_sets", "pcl_gd_winner"],
        ["pcl_gd_init_weight_sets", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals_images", "pcl_robust_weights_rows",
         "pcl_gd_winner"]),
    "images_robust_list_eager": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_gd_init_weight_sets",
         "pcl_gd_set_pano_groups", "pcl_gd_run_weight_sets", "pcl_gd_winner", "pcl_point_residuals_images", "pcl_robust_weights_rows",
         "pcl_gd_run_weight_sets", "pcl_gd_winner"],
        ["pcl_gd_init_weight_sets", "pcl_gd_set_pano_groups", "pcl_gd_run_weight_sets", "pcl_gd_winner", "pcl_point_residuals_images",
         "pcl_robust_weights_rows", "pcl_gd_run_weight_sets", "pcl_gd_winner"]),
    "images_shared": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "images_shared_eager": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner"]),
    "omniloc": (
        ["pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_result", "pcl_rot_from_ypr"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_result", "pcl_rot_from_ypr"]),
    "omniloc_all": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_result", "pcl_rot_from_ypr"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_result", "pcl_rot_from_ypr"]),
    "rooms": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "rooms_depth": (
        ["pcl_depth_default", "pcl_depth_default", "pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box",
         "pcl_quantile_box", "pcl_pano_pack_f16", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init_rooms_images", "pcl_gd_run_depth_chain",
         "pcl_gd_winner"],
        ["pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init_rooms_images", "pcl_gd_run_depth_chain",
         "pcl_gd_winner"]),
    "rooms_eager": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_run_rooms_images", "pcl_gd_winner"]),
    "rooms_images_depth": (
        ["pcl_depth_default", "pcl_depth_default", "pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box",
         "pcl_quantile_box", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_run_depth_chain", "pcl_gd_winner"],
        ["pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups",
         "pcl_gd_run_depth_chain", "pcl_gd_winner"]),
    "rooms_images_depth_prune": (
        ["pcl_depth_default", "pcl_depth_default", "pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box",
         "pcl_quantile_box", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_run_depth_chain", "pcl_gd_prune", "pcl_gd_run_depth_chain", "pcl_gd_winner"],
        ["pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups",
         "pcl_gd_run_depth_chain", "pcl_gd_prune", "pcl_gd_run_depth_chain", "pcl_gd_winner"]),
    "rooms_images_list": (
        ["pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_quantile_box", "pcl_quantile_box",
         "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "rooms_images_list_prune": (
        ["pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_quantile_box", "pcl_quantile_box",
         "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_winner"]),
    "rooms_images_shared": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "rooms_images_shared_eager": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner"]),
    "rooms_prune": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_init_rooms_images", "pcl_gd_prune",
         "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_winner"]),
    "rooms_prune_eager": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_prune", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_prune", "pcl_gd_run_rooms_images", "pcl_gd_winner"]),
}

# LADDERS: recorded on the MI355X from the parent of the commit that gave the images and the rooms entry points one ladder each
EXPECTED.update({
    "images_robust_one_image": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_run_weighted", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_winner"]),
    "images_sequential": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "one_set:images_list": (
        ["pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_pano_pack_f16", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "one_set:images_robust_list": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_run_weighted", "pcl_gd_winner", "pcl_pano_pack_f16",
         "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_winner", "pcl_gd_init",
         "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals", "pcl_robust_weights_rows", "pcl_gd_winner"]),
    "one_set:polished_list": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss", "pcl_pano_pack_f16", "pcl_cloud_pack", "pcl_gd_init",
         "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss", "pcl_gd_init",
         "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss"]),
    "one_set:rooms_images_list": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_cloud_pack", "pcl_cloud_pack",
         "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"],
        ["pcl_cloud_pack", "pcl_cloud_pack", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_cloud_pack",
         "pcl_cloud_pack", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "one_set:rooms_polished_list": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_quantile_box",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr",
         "pcl_cloud_pack", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner",
         "pcl_gn_refine_rooms", "pcl_rot_from_ypr"],
        ["pcl_cloud_pack", "pcl_cloud_pack", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms",
         "pcl_rot_from_ypr", "pcl_cloud_pack", "pcl_cloud_pack", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner",
         "pcl_gn_refine_rooms", "pcl_rot_from_ypr"]),
    "per_image:rooms_images_list": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_cloud_pack", "pcl_cloud_pack",
         "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"],
        ["pcl_cloud_pack", "pcl_cloud_pack", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_cloud_pack",
         "pcl_cloud_pack", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "per_image:rooms_images_shared": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_quantile_box", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_pano_pack_f16",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "per_image:rooms_polished": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_quantile_box",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr",
         "pcl_pano_pack_f16", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"]),
    "per_room:rooms_images_depth": (
        ["pcl_depth_default", "pcl_depth_default", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack",
         "pcl_depth_default", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner", "pcl_quantile_box", "pcl_cloud_order",
         "pcl_cloud_pack", "pcl_depth_default", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner"],
        ["pcl_depth_default", "pcl_depth_default", "pcl_depth_default", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner",
         "pcl_depth_default", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner"]),
    "polished_eager_gn": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"]),
    "polished_list_gn_cov": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_gd_init",
         "pcl_gd_set_pano_groups", "pcl_gd_run", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"]),
    "polished_one_image": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine", "pcl_rot_from_ypr", "pcl_sampling_loss"]),
    "polished_prune_gn": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_init", "pcl_gd_prune", "pcl_gd_run", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"]),
    "polished_robust_gn": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init_weight_sets",
         "pcl_gd_set_pano_groups", "pcl_gd_run_weight_sets", "pcl_gd_winner", "pcl_point_residuals_images", "pcl_robust_weights_rows",
         "pcl_gd_run_weight_sets", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"],
        ["pcl_gd_init_weight_sets", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_point_residuals_images", "pcl_robust_weights_rows",
         "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"]),
    "polished_shared_cov": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_winner", "pcl_pose_information_images"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_pose_information_images"]),
    "polished_shared_gn": (
        ["pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups",
         "pcl_gd_run", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_images", "pcl_rot_from_ypr"]),
    "room_cap:rooms": (
        ["pcl_quantile_box", "pcl_pano_pack_f16", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner", "pcl_quantile_box", "pcl_cloud_order", "pcl_cloud_pack", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_run",
         "pcl_gd_winner"],
        ["pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gd_init", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "room_cap:rooms_images": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_cloud_order", "pcl_cloud_pack", "pcl_quantile_box",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner"]),
    "room_cap:rooms_polished": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr", "pcl_cloud_order",
         "pcl_cloud_pack", "pcl_quantile_box", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner",
         "pcl_gn_refine_rooms", "pcl_rot_from_ypr"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"]),
    "rooms_polished_list_gn": (
        ["pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_cloud_order", "pcl_cloud_pack_sets", "pcl_pano_pack_f16", "pcl_pano_pack_f16",
         "pcl_quantile_box", "pcl_quantile_box", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner",
         "pcl_gn_refine_rooms", "pcl_rot_from_ypr"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"]),
    "rooms_polished_one_image": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_quantile_box", "pcl_quantile_box",
         "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"]),
    "rooms_polished_prune_cov": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box",
         "pcl_quantile_box", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_init_rooms_images",
         "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_pose_information_rooms"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_prune", "pcl_gd_winner", "pcl_pose_information_rooms"]),
    "rooms_polished_shared_gn_cov": (
        ["pcl_cloud_order", "pcl_cloud_pack", "pcl_cloud_order", "pcl_cloud_pack", "pcl_pano_pack_f16", "pcl_pano_pack_f16", "pcl_quantile_box",
         "pcl_quantile_box", "pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_run_rooms_images", "pcl_gd_winner", "pcl_gn_refine_rooms",
         "pcl_rot_from_ypr"],
        ["pcl_gd_init_rooms_images", "pcl_gd_set_pano_groups", "pcl_gd_winner", "pcl_gn_refine_rooms", "pcl_rot_from_ypr"]),
})


@pytest.mark.parametrize("name", sorted(PATHS))
def test_enqueue_sequence(monkeypatch, name):
    first, second = record(monkeypatch, name)
    print(name, first, second)
    assert first == EXPECTED[name][0], "first call (empty caches)"
    assert second == EXPECTED[name][1], "second call (cached packs, engine and graph)"


def _flat(x):
    if torch.is_tensor(x):
        return [x.detach().cpu().reshape(-1)]
    return [t for y in x for t in _flat(y)]


def outputs(name):
    """every tensor LADDERS[name] returns and every leaf tensor it wrote back, after one call from empty caches: one flat float32 CPU tensor"""
    from piccolo_amd import _lib
    from piccolo_amd import omniloc as po
    _lib.load()
    s = scene()
    with pytest.MonkeyPatch.context() as m:
        _force(m, name, po, s)
        po._cache.clear()
        got = torch.cat(_flat(LADDERS[name](po, s)))
        torch.cuda.synchronize()
        po._cache.clear()
    assert got.dtype == torch.float32
    return got


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_the_ladders_give_the_bits_recorded_before_they_were_merged(name):
    want = torch.from_numpy(load_golden("front_end_ladders.npz")[name])
    got = outputs(name)
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))         # (bits, so that a NaN covariance compares too)


if __name__ == "__main__":                 # python tests/test_enqueue_sequence.py OUT.npz: record the fixture
    import sys

    import numpy as np
    np.savez_compressed(sys.argv[1], **{name: outputs(name).numpy() for name in sorted(LADDERS)})
