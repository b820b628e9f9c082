"""GPU test of the kernel timer through every GD iteration loop: the single run (fused, two-launch, depth-masked), the rooms chain, the
rooms x images chain with colour sets and the depth chain.  A KernelTimer(capacity=2, stride=2) over five iterations brackets the loss
launches of iterations 0 and 2 — the capacity stops the one of iteration 4 — and timing changes nothing: result and loss history are
those of the same run without a timer, bit for bit."""
import pytest
import torch

from test_room_images import _per_image_colours
from test_room_images import _starts as _image_starts
from test_room_search import _query, _rooms

pytestmark = pytest.mark.gpu

SIZES = (4_000, 9_000)
RES = (64, 128)
PER_IMAGE = 6
N_ITER = 5
GD = dict(lr=0.1, patience=5, factor=0.8)
ROUTES = ["single_fused", "single_two_launch", "single_depth", "rooms", "rooms_images_sets", "depth_chain"]


@pytest.fixture(scope="module")
def scene():
    from piccolo_amd import ops
    rooms = _rooms(SIZES)
    return {"rooms": rooms, "sets": _per_image_colours(rooms, 2, seed=5), "boxes": [ops.quantile_box(x, 0.05) for x, _ in rooms],
            "panos": [ops.Pano(_query(rooms, r, 5 + r, res=RES)[0]) for r in (0, 1)], "starts": _image_starts(2, 2, PER_IMAGE, seed=5)}


def _engine(scene, route):
    """a fresh engine of the route, at its starting poses"""
    from piccolo_amd import ops
    rooms, boxes, panos, starts = scene["rooms"], scene["boxes"], scene["panos"], scene["starts"]
    if route.startswith("single"):
        tr, ro = starts[1][0]
        kw = {"single_fused": {}, "single_two_launch": dict(fuse=False), "single_depth": dict(depth_mask=True)}[route]
        return ops.GradientDescent(ops.Cloud(*rooms[1]), panos[0], tr, ro, boxes[1], **GD, **kw)
    if route == "rooms_images_sets":
        clouds = [ops.Cloud.with_color_sets(x, cols) for x, cols in scene["sets"]]
        tr = torch.cat([starts[r][i][0] for r in (0, 1) for i in (0, 1)])
        ro = torch.cat([starts[r][i][1] for r in (0, 1) for i in (0, 1)])
        return ops.GradientDescentRoomsImages(list(zip(clouds, boxes)), panos, tr, ro, **GD)
    tr, ro = torch.cat([starts[r][0][0] for r in (0, 1)]), torch.cat([starts[r][0][1] for r in (0, 1)])
    return ops.GradientDescentRooms(list(zip([ops.Cloud(*rm) for rm in rooms], boxes)), panos[0], tr, ro, **GD, depth_mask=route == "depth_chain")


def _fused(gd):
    import ctypes
    from piccolo_amd import _lib
    if hasattr(gd, "plan"):
        return bool(gd.plan()[2])
    f = ctypes.c_int(-1)
    assert _lib.load().pcl_gd_plan_hyper(gd.cloud.n, gd.B, ctypes.byref(gd.hyper), None, None, ctypes.byref(f)) == 0
    return bool(f.value)


@pytest.mark.parametrize("route", ROUTES)
def test_timer_counts_two_launches_and_changes_nothing(scene, route):
    from piccolo_amd import ops
    plain = _engine(scene, route)
    # (the routes are the loops' forms: one launch per iteration where every block is resident, two launches elsewhere)
    assert _fused(plain) == (route in ("single_fused", "rooms", "rooms_images_sets"))
    want_hist = plain.run(N_ITER, history=True)
    want = plain.result()
    assert bool(torch.isfinite(want_hist).all())

    timer = ops.KernelTimer(capacity=2, stride=2)
    gd = _engine(scene, route)
    hist = gd.run(N_ITER, history=True, timer=timer)
    ms, launches = timer.read()
    # (pcl_timer_read hands back a count and a sum, not which iterations were timed.  That the two are iterations 0 and 2 follows from
    #  this count together with the capacity-8 run at the end: a stride that is ignored times 0 and 1 here but all 5 there, one counted
    #  in recorded pairs stops after iteration 0 here; only "every second iteration, while slots remain" gives 2 here and 3 there)
    assert launches == 2 and ms > 0.0, (launches, ms)
    assert torch.equal(hist, want_hist) and torch.equal(gd.result(), want)
    timer.reset()
    assert timer.read() == (0.0, 0)
    gd.run(N_ITER, timer=timer)
    ms, launches = timer.read()
    assert launches == 2 and ms > 0.0, (launches, ms)
    # room for every timed iteration: 0, 2 and 4 (the stride is counted in iterations, not in recorded pairs)
    wide = ops.KernelTimer(capacity=8, stride=2)
    gd.run(N_ITER, timer=wide)
    assert wide.read()[1] == 3
