"""CPU checks of the workspace layouts behind the loss and GD entry points: every size query answers the byte count it has always
answered (a table of literals, recorded from the library before the layouts were gathered into one carve per family), the plan
queries likewise, and every run entry point refuses a workspace one byte below its query — before anything touches a device."""
import ctypes

import pytest

from test_room_search_abi import DUMMY, SHAPES, _hyper, _rooms

VP = ctypes.c_void_p
H, W = 1024, 2048
RI_ROOMS, RI_IMAGES, RI_PER = (700, 120_000, 166_667), 2, 6             # the rooms x images shape
GD_SHAPES = [(166_667, 6, {}), (1_000_000, 32, {}), (120_000, 24, dict(color_sets=3)),
             (1_000_000, 32, dict(depth_mask=1)), (1_000_000, 32, dict(depth_mask=1, depth_stride=1))]


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def _ints(k):
    return (ctypes.c_int * k)(*([-1] * k))


def _measure(lib):
    """every pinned figure, by name: sizes as integers, plans as (nchunks..., G, fused) tuples"""
    out = {}
    out["loss 1025x4"] = lib.pcl_loss_workspace_bytes(1025, 4)
    for stride in (0, 1):
        out["loss_depth 1025x4 64x128 stride %d" % stride] = lib.pcl_loss_depth_workspace_bytes(1025, 4, 64, 128, 0, 0, stride)
        # (1025 points resolve the same default grid at both strides; at 1M points the grid follows the stride: 144 x 288 / 200 x 400)
        out["loss_depth 1000000x32 stride %d" % stride] = lib.pcl_loss_depth_workspace_bytes(1_000_000, 32, H, W, 0, 0, stride)
    for n, B, kw in GD_SHAPES:
        h = _hyper(**kw)
        key = "gd %dx%d %s" % (n, B, sorted(kw.items()))
        out[key] = lib.pcl_gd_workspace_bytes(n, B, H, W, ctypes.byref(h))
        c, g, f = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.pcl_gd_plan_hyper(n, B, ctypes.byref(h), ctypes.byref(c), ctypes.byref(g), ctypes.byref(f)) == 0
        out["plan " + key] = (c.value, g.value, f.value)
    for sizes, per_room in SHAPES:
        h, key = _hyper(), "rooms %s x %d" % (sizes, per_room)
        out[key] = lib.pcl_gd_rooms_workspace_bytes(_rooms(sizes), len(sizes), per_room, ctypes.byref(h))
        nch, g, f = _ints(len(sizes)), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.pcl_gd_plan_rooms(_rooms(sizes), len(sizes), per_room, ctypes.byref(h), nch, ctypes.byref(g), ctypes.byref(f)) == 0
        out["plan " + key] = (*nch, g.value, f.value)
    rooms = _rooms(RI_ROOMS)
    for sets in (0, 2):
        h, key = _hyper(color_sets=sets), "rooms_images color_sets %d" % sets
        out[key] = lib.pcl_gd_rooms_images_workspace_bytes(rooms, len(RI_ROOMS), RI_IMAGES, RI_PER, ctypes.byref(h))
        nch, g, f = _ints(len(RI_ROOMS)), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.pcl_gd_plan_rooms_images(rooms, len(RI_ROOMS), RI_IMAGES, RI_PER, ctypes.byref(h), nch, ctypes.byref(g), ctypes.byref(f)) == 0
        out["plan " + key] = (*nch, g.value, f.value)
        h, key = _hyper(color_sets=sets, depth_mask=1), "depth_chain color_sets %d" % sets
        out[key] = lib.pcl_gd_depth_chain_workspace_bytes(rooms, len(RI_ROOMS), RI_IMAGES, RI_PER, H, W, ctypes.byref(h))
        nch, g, dh, dw, st = _ints(len(RI_ROOMS)), ctypes.c_int(-1), _ints(len(RI_ROOMS)), _ints(len(RI_ROOMS)), _ints(len(RI_ROOMS))
        assert lib.pcl_gd_plan_depth_chain(rooms, len(RI_ROOMS), RI_IMAGES, RI_PER, H, W, ctypes.byref(h), nch, ctypes.byref(g), dh, dw, st) == 0
        out["plan " + key] = (*nch, g.value, *dh, *dw, *st)
    h = _hyper(depth_mask=1)
    out["depth_chain 1 room x 1 image"] = lib.pcl_gd_depth_chain_workspace_bytes(_rooms((166_667,)), 1, 1, 6, H, W, ctypes.byref(h))
    nch, g = _ints(1), ctypes.c_int(-1)
    assert lib.pcl_gd_plan_depth_chain(_rooms((166_667,)), 1, 1, 6, H, W, ctypes.byref(h), nch, ctypes.byref(g), None, None, None) == 0
    out["plan depth_chain 1 room x 1 image"] = (*nch, g.value)
    return out


PINNED = {
    'loss 1025x4': 1280,
    'loss_depth 1025x4 64x128 stride 0': 9472,
    'loss_depth 1025x4 64x128 stride 1': 9472,
    'loss_depth 1000000x32 stride 0': 5572608,
    'loss_depth 1000000x32 stride 1': 10504192,
    'gd 166667x6 []': 125952,
    'plan gd 166667x6 []': (328, 2, 1),
    'gd 1000000x32 []': 524288,
    'plan gd 1000000x32 []': (256, 2, 0),
    "gd 120000x24 [('color_sets', 3)]": 368640,
    "plan gd 120000x24 [('color_sets', 3)]": (240, 2, 0),
    "gd 1000000x32 [('depth_mask', 1)]": 11141120,
    "plan gd 1000000x32 [('depth_mask', 1)]": (256, 2, 0),
    "gd 1000000x32 [('depth_mask', 1), ('depth_stride', 1)]": 21004288,
    "plan gd 1000000x32 [('depth_mask', 1), ('depth_stride', 1)]": (256, 2, 0),
    'rooms (700, 120000, 166667) x 6': 223232,
    'plan rooms (700, 120000, 166667) x 6': (8, 240, 328, 2, 0),
    'rooms (166667, 166667, 166667, 166667, 166667, 166667, 166667, 166667) x 6': 1009664,
    'plan rooms (166667, 166667, 166667, 166667, 166667, 166667, 166667, 166667) x 6': (328, 328, 328, 328, 328, 328, 328, 328, 2, 0),
    'rooms (1000000, 1000000, 1000000, 1000000) x 32': 2099200,
    'plan rooms (1000000, 1000000, 1000000, 1000000) x 32': (256, 256, 256, 256, 2, 0),
    'rooms (50, 3000, 2500000) x 5': 270848,
    'plan rooms (50, 3000, 2500000) x 5': (8, 8, 824, 1, 0),
    'rooms (166667,) x 6': 128000,
    'plan rooms (166667,) x 6': (328, 2, 1),
    'rooms (4096, 4097, 10000, 300000, 1000000) x 1': 108544,
    'plan rooms (4096, 4097, 10000, 300000, 1000000) x 1': (8, 16, 24, 592, 1024, 1, 0),
    'rooms_images color_sets 0': 444416,
    'plan rooms_images color_sets 0': (8, 240, 328, 2, 0),
    'depth_chain color_sets 0': 2288896,
    'plan depth_chain color_sets 0': (8, 240, 328, 2, 16, 64, 80, 32, 128, 160, 1, 1, 1),
    'rooms_images color_sets 2': 444416,
    'plan rooms_images color_sets 2': (8, 240, 328, 2, 0),
    'depth_chain color_sets 2': 2288896,
    'plan depth_chain color_sets 2': (8, 240, 328, 2, 16, 64, 80, 32, 128, 160, 1, 1, 1),
    'depth_chain 1 room x 1 image': 740352,
    'plan depth_chain 1 room x 1 image': (328, 2),
}


def test_size_and_plan_queries_answer_the_pinned_figures(lib):
    got = _measure(lib)
    assert sorted(got) == sorted(PINNED)
    wrong = {k: (v, PINNED[k]) for k, v in got.items() if v != PINNED[k]}
    assert not wrong, wrong
    assert all(v for v in got.values())                                   # (no shape of the table is a refused one)
    # the one-room, one-image depth chain is handed to pcl_gd_run: its query covers that workspace as well
    h = _hyper(depth_mask=1)
    assert got["depth_chain 1 room x 1 image"] >= lib.pcl_gd_workspace_bytes(166_667, 6, H, W, ctypes.byref(h))


def test_every_run_refuses_a_workspace_one_byte_below_its_query(lib):
    """PCL_EWORKSPACE (-2) with dummy non-null device addresses: the refusal comes before any HIP call (this runs without a GPU).  The
    other direction is the GPU suite's: the engines of ops.py allocate exactly the query."""
    from piccolo_amd import _lib
    d, fmt = VP(DUMMY), _lib.PANO_F16
    need = lib.pcl_loss_workspace_bytes(1025, 4)
    assert need > 0 and lib.pcl_sampling_loss(d, 1025, d, fmt, 64, 128, d, d, 4, 1, None, d, d, need - 1, None) == -2
    for stride in (0, 1):
        need = lib.pcl_loss_depth_workspace_bytes(1025, 4, 64, 128, 0, 0, stride)
        assert need > 0 and lib.pcl_sampling_loss_depth(d, 1025, d, fmt, 64, 128, d, d, 4, 1, 0, 0, 0.05, stride, d, d, need - 1, None) == -2
        need = lib.pcl_loss_depth_workspace_bytes(1_000_000, 32, H, W, 0, 0, stride)
        assert need > 0 and lib.pcl_sampling_loss_depth(d, 1_000_000, d, fmt, H, W, d, d, 32, 1, 0, 0, 0.05, stride, d, d, need - 1, None) == -2
    for n, B, kw in GD_SHAPES:                                            # plain, colour sets, depth mask
        h = _hyper(**kw)
        need = lib.pcl_gd_workspace_bytes(n, B, H, W, ctypes.byref(h))
        assert need > 0 and lib.pcl_gd_run(d, n, d, fmt, H, W, d, B, d, ctypes.byref(h), 3, None, d, need - 1, None, None) == -2, (n, B, kw)
    for sizes, per_room in SHAPES:
        h, rooms = _hyper(), _rooms(sizes)
        need = lib.pcl_gd_rooms_workspace_bytes(rooms, len(sizes), per_room, ctypes.byref(h))
        assert need > 0 and lib.pcl_gd_run_rooms(rooms, len(sizes), d, fmt, 64, 128, d, per_room, ctypes.byref(h), 3, None, d, need - 1, None, None) == -2
    rooms, shape = _rooms(RI_ROOMS), (len(RI_ROOMS), RI_IMAGES)
    for sets in (0, 2):
        h = _hyper(color_sets=sets)
        need = lib.pcl_gd_rooms_images_workspace_bytes(rooms, *shape, RI_PER, ctypes.byref(h))
        assert need > 0 and lib.pcl_gd_run_rooms_images(rooms, *shape, d, fmt, H, W, d, RI_PER, ctypes.byref(h), 3, None, d, need - 1, None, None) == -2
        h = _hyper(color_sets=sets, depth_mask=1)
        need = lib.pcl_gd_depth_chain_workspace_bytes(rooms, *shape, RI_PER, H, W, ctypes.byref(h))
        assert need > 0 and lib.pcl_gd_run_depth_chain(rooms, *shape, d, fmt, H, W, d, RI_PER, ctypes.byref(h), 3, None, d, need - 1, None, None) == -2
    h, one = _hyper(depth_mask=1), _rooms((166_667,))
    need = lib.pcl_gd_depth_chain_workspace_bytes(one, 1, 1, 6, H, W, ctypes.byref(h))
    assert need > 0 and lib.pcl_gd_run_depth_chain(one, 1, 1, d, fmt, H, W, d, 6, ctypes.byref(h), 3, None, d, need - 1, None, None) == -2
