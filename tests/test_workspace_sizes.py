"""CPU checks of the workspace layouts behind the loss, GD and initialisation-stage entry points: every size query answers the byte
count it has always answered (a table of literals, recorded from the library before the layouts were gathered into one carve per
family), the plan queries likewise, and every run entry point refuses a workspace one byte below its query — before anything
touches a device."""
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


# the initialisation stage (histogram trim, loss trim, work list) and the colour / packing workspaces: (points, candidates, H, W); every
# histogram shape on 4 x 4 blocks.  The last panorama has 65 x 65 = 4225 tiles of 64 px: the tile-binned render is refused and the
# render area of the n-sized workspace falls back to the z-buffer's size.
INIT_SHAPES = [(1025, 4, 64, 128), (166_667, 50, 1024, 2048), (1_000_000, 64, 1024, 2048), (166_667, 4, 4160, 4160)]
INIT_IMAGES = 4                                                            # images (and colour sets) of the several-image queries
TRIM_SHAPES = [(1025, 4, 2), (166_667, 50, 6), (1_000_000, 64, 6)]        # (points, translations, rotation groups)


def _measure_init(lib):
    out = {}
    for n, K, h, w in INIT_SHAPES:
        key = "%dx%d %dx%d" % (n, K, h, w)
        out["hist " + key] = lib.pcl_hist_trim_workspace_bytes(K, h, w, 4, 4)
        out["hist_n " + key] = lib.pcl_hist_trim_workspace_bytes_n(n, K, h, w, 4, 4)
        out["hist_images %d x " % INIT_IMAGES + key] = lib.pcl_hist_trim_images_workspace_bytes(n, INIT_IMAGES, K, h, w, 4, 4)
        for npts, sets in ((0, 1), (n, 1), (n, INIT_IMAGES)):
            out["hist_images_sets n %d sets %d: %d x %s" % (npts, sets, INIT_IMAGES, key)] = lib.pcl_hist_trim_images_sets_workspace_bytes(
                npts, sets, INIT_IMAGES, K, h, w, 4, 4)
    for n, K, g in TRIM_SHAPES:
        key = "%dx%dx%d" % (n, K, g)
        out["trim " + key] = lib.pcl_trim_loss_workspace_bytes(n, K, g)
        for images in (8, 32):
            out["trim_images %d x " % images + key] = lib.pcl_trim_loss_images_workspace_bytes(n, K, g, images)
        out["trim_order " + key] = lib.pcl_trim_order_bytes(n, K, g)
    # (pcl_trim_order_workspace_bytes, pcl_cloud_order_workspace_bytes and pcl_color_template_workspace_bytes end in rocprim's temporary
    #  storage, whose size query depends on the device it finds — none without one: not figures a table of literals can hold)
    out["color_ws"] = lib.pcl_color_workspace_bytes()
    for c in (8, 256):
        out["histogram_ws %d^3" % c] = lib.pcl_histogram_workspace_bytes(c, c, c)
    return out


PINNED_INIT = {
    'hist 1025x4 64x128': 360704,
    'hist_n 1025x4 64x128': 371200,
    'hist_images 4 x 1025x4 64x128': 1477888,
    'hist_images_sets n 0 sets 1: 4 x 1025x4 64x128': 1442816,
    'hist_images_sets n 1025 sets 1: 4 x 1025x4 64x128': 1477888,
    'hist_images_sets n 1025 sets 4: 4 x 1025x4 64x128': 1484800,
    'hist 166667x50 1024x2048': 839716096,
    'hist_n 166667x50 1024x2048': 842146816,
    'hist_images 4 x 166667x50 1024x2048': 3367586048,
    'hist_images_sets n 0 sets 1: 4 x 166667x50 1024x2048': 3358863872,
    'hist_images_sets n 166667 sets 1: 4 x 166667x50 1024x2048': 3367586048,
    'hist_images_sets n 166667 sets 4: 4 x 166667x50 1024x2048': 3368586752,
    'hist 1000000x64 1024x2048': 1074827264,
    'hist_n 1000000x64 1024x2048': 3206157568,
    'hist_images 4 x 1000000x64 1024x2048': 12818629888,
    'hist_images_sets n 0 sets 1: 4 x 1000000x64 1024x2048': 4299309056,
    'hist_images_sets n 1000000 sets 1: 4 x 1000000x64 1024x2048': 12818629888,
    'hist_images_sets n 1000000 sets 4: 4 x 1000000x64 1024x2048': 12824630272,
    'hist 166667x4 4160x4160': 553877760,
    'hist_n 166667x4 4160x4160': 571516928,
    'hist_images 4 x 166667x4 4160x4160': 2285067008,
    'hist_images_sets n 0 sets 1: 4 x 166667x4 4160x4160': 2215511040,
    'hist_images_sets n 166667 sets 1: 4 x 166667x4 4160x4160': 2285067008,
    'hist_images_sets n 166667 sets 4: 4 x 166667x4 4160x4160': 2286067712,
    'trim 1025x4x2': 2560,
    'trim_images 8 x 1025x4x2': 16896,
    'trim_images 32 x 1025x4x2': 66048,
    'trim_order 1025x4x2': 512,
    'trim 166667x50x6': 633600,
    'trim_images 8 x 166667x50x6': 4934400,
    'trim_images 32 x 166667x50x6': 19680000,
    'trim_order 166667x50x6': 77056,
    'trim 1000000x64x6': 1597440,
    'trim_images 8 x 1000000x64x6': 12607488,
    'trim_images 32 x 1000000x64x6': 50356224,
    'trim_order 1000000x64x6': 196864,
    'color_ws': 58624,
    'histogram_ws 8^3': 2304,
    'histogram_ws 256^3': 67109120,
}


def test_initialisation_stage_queries_answer_the_pinned_figures(lib):
    got = _measure_init(lib)
    assert sorted(got) == sorted(PINNED_INIT)
    wrong = {k: (v, PINNED_INIT[k]) for k, v in got.items() if v != PINNED_INIT[k]}
    assert not wrong, wrong
    assert all(v for v in got.values())
    n, K, h, w = INIT_SHAPES[-1]                                          # no tile-binned render: the n-sized query adds the masks and codes only
    key = "%dx%d %dx%d" % (n, K, h, w)
    assert got["hist_n " + key] - got["hist " + key] == ((h * w + 255) // 256 + (2 * n + 255) // 256) * 256


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


def test_initialisation_stage_runs_refuse_a_workspace_one_byte_below_their_query(lib):
    """The histogram entry refuses below its SMALL (n = 0) query — anything between that and the n-sized one selects the z-buffer splat."""
    from piccolo_amd import _lib
    d, fmt = VP(DUMMY), _lib.PANO_U8
    ptrs = (VP * INIT_IMAGES)(*([DUMMY] * INIT_IMAGES))
    for n, K, h, w in INIT_SHAPES:
        for sets in (1, INIT_IMAGES):
            need = lib.pcl_hist_trim_images_sets_workspace_bytes(0, sets, INIT_IMAGES, K, h, w, 4, 4)
            assert need > 0 and lib.pcl_hist_trim_scores_images_sets(d, n, sets, ptrs, INIT_IMAGES, K, h, w, d, d, 4, 4, d, d, d, d, need - 1, None) == -2
    for n, K, g in TRIM_SHAPES:
        for sets in (1, INIT_IMAGES):
            need = lib.pcl_trim_loss_images_workspace_bytes(n, K, g, INIT_IMAGES)
            assert need > 0 and lib.pcl_trim_loss_images_sets(d, n, sets, ptrs, INIT_IMAGES, fmt, H, W, d, K, d, 4 * g, d, g, None, d, None, d, need - 1,
                                                              None) == -2
        need = lib.pcl_trim_order_workspace_bytes(n, K, g)
        assert need > 0 and lib.pcl_trim_order(d, n, fmt, H, W, d, K, d, 4 * g, d, g, d, d, need - 1, None) == -2
