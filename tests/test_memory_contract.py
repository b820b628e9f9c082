"""The memory contract of the library's entry points (README: what they return "depends on their arguments only"; DESIGN.md "Memory
contract"): no read of memory the library has not written itself, no write outside the queried bytes, every returned element defined.

Every scenario builds all it needs (clouds, panoramas, trim groups, engines, templates) and returns a flat dict of every tensor its caller
can see.  It runs four times — unpatched, and with every allocation of piccolo_amd/ops.py guarded and poisoned by each of the three fill
words of ws_helpers — and the four results must be bit-identical, the guards intact, the ledgers non-empty and alike.  The census at the
end holds the union of the recorded callers against the `_bytes(` call sites of ops.py.

The harness itself is tested on the CPU (plain torch ops standing in for kernels), and once more on CUDA tensors."""
import numpy as np
import pytest
import torch

import ws_helpers as ws

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------- the harness, on the CPU
N_WS = 64                  # bytes of the stand-ins' workspace


def _standin(kind, init):
    """a stand-in for an entry point: allocates as ops.py does, `init`: writes what it reads first (the correct twin)"""
    from piccolo_amd import ops
    buf = ops._bytes(N_WS)
    out = ops.torch.empty(2, dtype=torch.float32, device="cpu")
    out.zero_()
    if kind == "sum":                               # sums its whole workspace
        f = buf.view(torch.float32)
        if init:
            f.zero_()
        out[0] = f.sum()
    elif kind == "positive":                        # reads the workspace only through x > 0
        f = buf.view(torch.float32)
        if init:
            f.zero_()
        out[0] = float((f > 0).sum())
    elif kind == "min_u64":                         # a z-buffer: min over u64 words against a key below every non-zero fill
        q = buf.view(torch.int64)
        if init:
            q.fill_(-1)
        key = 0x3F000000_00000007
        words = [int(v) & 0xFFFFFFFFFFFFFFFF for v in q.tolist()]
        out[0] = float(min(words + [key]) == key)
    return {"out": out.clone()}


def _caught(kind):
    with ws.poisoned(0, device="cpu"):
        ref = _standin(kind, True)
    runs = ws.poisoned_runs(lambda: _standin(kind, False), device="cpu")
    return ref, runs, {w for w, r in runs.items() if ws.differences(ref, r.result)}


def test_harness_catches_a_read_of_the_whole_workspace():
    ref, runs, caught = _caught("sum")
    assert caught == {0xFFFFFFFF, 0x3F800000}       # (a sum of zeros is the correct twin's)
    assert len({tuple(r.result["out"].view(torch.int32).tolist()) for r in runs.values()}) == 3
    with pytest.raises(AssertionError, match="changes"):
        ws.assert_contract(ref, runs)


def test_harness_passes_a_stand_in_that_writes_before_it_reads():
    with ws.poisoned(0, device="cpu"):
        ref = _standin("sum", True)
    runs = ws.poisoned_runs(lambda: _standin("sum", True), device="cpu")
    ws.assert_contract(ref, runs)
    assert [k for k, _ in runs[0].callers] == ["bytes", "empty"] and all(c[0] == "_standin" for _, c in runs[0].callers)


def test_harness_comparison_mask_is_caught_by_the_finite_word_alone():
    assert _caught("positive")[2] == {0x3F800000}


def test_harness_u64_min_is_caught_by_the_zero_word_alone():
    assert _caught("min_u64")[2] == {0x00000000}


def _overrun(device, where):
    """one byte written through the base at interior offset `where` (-1: the head guard's last byte; N_WS: the tail guard's first)"""
    from piccolo_amd import ops
    with ws.poisoned(0xFFFFFFFF, device=device) as ledger:
        buf = ops._bytes(N_WS)
        other = ops.torch.empty(3, 5, dtype=torch.int64, device=device)
        assert buf.numel() == N_WS and other.shape == (3, 5) and other.dtype == torch.int64 and bool((other == -1).all())
        assert buf.data_ptr() % 512 == ledger[0].base.data_ptr() % 512            # the guard keeps the allocator's alignment
        ledger[0].base[ws.GUARD + where] = 0
        ws.check_guards()


@pytest.mark.parametrize("where", [N_WS, -1])
def test_harness_names_the_caller_of_a_damaged_guard(where):
    with pytest.raises(AssertionError, match=r"bytes of _overrun:\d+ \(64 bytes\) wrote at offset %d$" % where):
        _overrun("cpu", where)


def test_harness_passes_a_write_of_the_last_interior_byte():
    _overrun("cpu", N_WS - 1)


def test_harness_fills_and_restores():
    from piccolo_amd import ops
    real_bytes, real_torch = ops._bytes, ops.torch
    with ws.poisoned(0x3F800000, device="cpu") as ledger:
        t = ops._bytes(7)                             # at least 16 bytes, as ops._bytes
        assert t.numel() == 16 and bool((t.view(torch.float32) == 1.0).all())
        h = ops.torch.empty((3,), dtype=torch.float16, device="cpu")            # 6 bytes: a word and the low bytes of one
        assert h.view(torch.uint8).tolist() == [0x00, 0x00, 0x80, 0x3F, 0x00, 0x00]
        assert ops.torch.empty(0, dtype=torch.float32, device="cpu").numel() == 0
        assert [e.n for e in ledger] == [16, 6, 0] and [e.kind for e in ledger] == ["bytes", "empty", "empty"]
        assert all(e.base.numel() == 2 * ws.GUARD + e.n for e in ledger)
        p = ops.torch
        assert p.is_tensor is torch.is_tensor and p.cuda is torch.cuda and p.Tensor is torch.Tensor and p.float32 is torch.float32
        assert p.equal is torch.equal and p.zeros is torch.zeros
        ws.check_guards()
    assert ops._bytes is real_bytes and ops.torch is real_torch and ops.torch is torch
    with pytest.raises(ZeroDivisionError):
        with ws.poisoned(0, device="cpu"):
            1 / 0
    assert ops._bytes is real_bytes and ops.torch is real_torch


def test_same_bits_and_flat():
    nan = torch.tensor([float("nan"), 1.0])
    assert ws.same_bits(nan, nan.clone()) and not ws.same_bits(nan, -nan) and not ws.same_bits(nan, nan.double())
    assert not ws.same_bits(torch.zeros(2), torch.zeros(1, 2)) and ws.same_bits(torch.tensor(3), torch.tensor(3))
    assert ws.same_bits(None, None) and not ws.same_bits(None, nan) and ws.same_bits([nan, 2], (nan, 2)) and not ws.same_bits(0.0, -0.0)
    import types
    assert ws.same_bits("l1", "l1") and not ws.same_bits("l1", "l2") and not ws.same_bits(1, "1")
    d = ws.flat({"a": [nan, types.SimpleNamespace(**{"0": nan, "1": None})], "b": 2})
    assert sorted(d) == ["a.0", "a.1.0", "a.1.1", "b"]
    assert ws.differences(d, dict(d)) == [] and ws.differences(d, {"b": 2}) == ["a.0", "a.1.0", "a.1.1"]


ALLOWED = {
    # (at most two (function, line) sites with their reasons; none is needed: the allocation ladder's last resort is reached by a
    # refusing _bytes, scenario hist_last_resort)
}


def test_the_walk_finds_the_call_sites():
    sites = ws.bytes_sites()
    assert len(sites) >= 30, sites
    names = {f for f, _ in sites}
    assert {"_order_and_buffer", "sampling_loss", "_gauss_newton", "_hist_workspace", "_allocate", "_robust_buffers", "make_pano"} <= names
    assert "_bytes" not in names and len(ALLOWED) <= 2 and set(ALLOWED) <= set(sites)


# ------------------------------------------------------------------------------------------------- scenes (inputs: built once, outside)
def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def S(oracle, name):
    from test_point_weights import scene
    return scene(oracle, name)


_PANO31 = {}


def img31(oracle):
    """S1's scene on a 31-row panorama: the last half pair of the u8p / u8v layouts"""
    if not _PANO31:
        from piccolo_amd import synth
        xyz, rgb = S(oracle, "S1B4")[:2]
        t_gt, ypr_gt = synth.gt_pose(1025 % 97)
        _PANO31["img"] = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb, (31, 64)).astype(np.float32) / 255
    return _PANO31["img"]


def second_image(img):
    """another k/255 image of the same size: the first one mirrored, its channels rotated"""
    return np.ascontiguousarray(img[:, ::-1, ::-1])


def weights_of(n, seed=3):
    return np.array([0.0, 0.3, 1.0, 1.7, 4.5], np.float32)[np.random.default_rng(seed).integers(0, 5, size=n)]


def cloud_fields(c):
    return {"data": c.data, "order": c.order, "weights": c.weights}


SEEN = {}                   # scenario -> the ("bytes" | "empty", caller) pairs its scenarios recorded


def run(name, scenario, **kw):
    """the four runs of a scenario and what they must show"""
    ws.clear_caches()
    ref = scenario()
    torch.cuda.synchronize()
    runs = ws.poisoned_runs(scenario, **kw)
    SEEN.setdefault(name, set()).update(runs[ws.FILL_WORDS[0]].callers)
    ws.assert_contract(ref, runs)


# ------------------------------------------------------------------------------------------------- 1. packing
def packing(oracle):
    from piccolo_amd import ops
    out = {}
    xyz, rgb, img, trans, rot = S(oracle, "S1B4")
    X, C = T(xyz), T(rgb)
    plain = ops.Cloud(X, C)
    out["sorted"] = cloud_fields(plain)
    out["unsorted"] = cloud_fields(ops.Cloud(X, C, sort=False))
    out["weighted"] = cloud_fields(ops.Cloud(X, C, weights=T(weights_of(len(xyz)))))
    out["one"] = cloud_fields(ops.Cloud(X[:1].contiguous(), C[:1].contiguous()))
    sets = ops.Cloud.with_color_sets(X, [C, C.flip(1).contiguous(), (0.5 * C).contiguous()])
    out["sets"] = cloud_fields(sets)
    # coordinates whose 2 x 2 footprints touch all four borders, the corners among them
    g = torch.linspace(-1.1, 1.1, 23, device="cuda")
    coord = torch.stack(torch.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).contiguous()
    # poses that look at the poles (pitch +- pi / 2) next to level ones, from the room's middle
    pole = T(np.array([[0, 0, 0], [1.0, np.pi / 2, 0], [2.0, -np.pi / 2, 0.3], [0.5, np.pi / 2, 0.3], [3.0, 1.2, -1.0]], np.float32))
    groups = ops.TrimGroups(pole)
    for H, im in ((32, img), (31, img31(oracle))):
        I = T(im)
        for fmt in ("f32", "u8", "f16"):
            pano = ops.Pano(I, fmt=fmt)
            out["texels.%d.%s" % (H, fmt)] = pano.data               # the bordered texture itself: every border texel and pad is written
            out["sample.%d.%s" % (H, fmt)] = ops.sample_from_img(pano, coord)
        for fmt in ("u8p", "u8v", "u8"):
            pano = ops.Pano(I, fmt=fmt)
            out["texels.%d.%s.trim" % (H, fmt)] = pano.data
            out["pole.%d.%s" % (H, fmt)] = ops.trim_loss_table(plain, pano, T(trans), groups, return_count=True)
        out["auto.%d" % H] = ops.sample_from_img(ops.Pano(I), coord)
        out["float.%d" % H] = ops.sample_from_img(ops.Pano(I * 0.3), coord)            # not k/255: the f32 fallback of "auto"
    return ws.flat(out)


@gpu
def test_packing(oracle):
    run("packing", lambda: packing(oracle))


# ------------------------------------------------------------------------------------------------- 2. loss
def loss(oracle):
    from piccolo_amd import ops
    out = {}
    for name in ("S1B4", "S1B3", "S2"):
        xyz, rgb, img, trans, rot = S(oracle, name)
        n, B = len(xyz), len(trans)
        X, C, I, tr, ro = T(xyz), T(rgb), T(img), T(trans), T(rot)
        cloud = ops.Cloud(X, C)
        wcloud = ops.Cloud(X, C, order=cloud.order, weights=T(weights_of(n)))
        vis = T((np.random.default_rng(5).random((B, n)) >= 0.4).astype(np.uint8))
        for fmt in ("f16", "u8", "f32") if name == "S1B4" else ("f16",):
            pano = ops.Pano(I, fmt=fmt)
            k = "%s.%s." % (name, fmt)
            for grad in (True, False):
                out[k + "loss.%d" % grad] = ops.sampling_loss(cloud, pano, tr, ro, with_grad=grad)
                out[k + "visible.%d" % grad] = ops.sampling_loss(cloud, pano, tr, ro, with_grad=grad, visible=vis)
                out[k + "weighted.%d" % grad] = ops.sampling_loss(wcloud, pano, tr, ro, with_grad=grad)
                out[k + "depth.%d" % grad] = ops.sampling_loss(cloud, pano, tr, ro, with_grad=grad, depth=True)
            out[k + "depth.grid"] = ops.sampling_loss(cloud, pano, tr, ro, depth=dict(depth_res=(16, 32), depth_stride=2))
            out[k + "residuals"] = ops.point_residuals(cloud, pano, tr, ro)
            packed = ops.point_residuals(cloud, pano, tr, ro, packed=True)
            out[k + "residuals.packed"] = packed
            panos = [pano, ops.Pano(T(second_image(img)), fmt=fmt)]
            out[k + "residuals.images"] = ops.point_residuals_images(cloud, panos, tr[:2], ro[:2])
            for kind in ("trunc", "huber"):
                out[k + "robust." + kind] = ops.robust_weights(cloud, packed[0], kind=kind)
                out[k + "robust.rows." + kind] = ops.robust_planes(n, packed, kind=kind, k=1.5)
        out[name + ".mask"] = ops.depth_mask(cloud, tr, ro, (16, 32))
        out[name + ".mask.stride"] = ops.depth_mask(cloud, tr, ro, (17, 33), tau=0.05, stride=2)
    return ws.flat(out)


@gpu
def test_loss(oracle):
    run("loss", lambda: loss(oracle))


# ------------------------------------------------------------------------------------------------- 3. information and polish
def polish(oracle):
    from piccolo_amd import ops
    out = {}
    for name in ("S1B4", "S1B3", "S2"):
        xyz, rgb, img, trans, rot = S(oracle, name)
        n = len(xyz)
        X, C, I, tr, ro = T(xyz), T(rgb), T(img), T(trans), T(rot)
        cloud, pano = ops.Cloud(X, C), ops.Pano(I, fmt="f16")
        panos = [pano, ops.Pano(T(second_image(img)), fmt="f16")]
        wcloud = ops.Cloud(X, C, order=cloud.order, weights=T(weights_of(n) + 0.25))
        out[name + ".info"] = ops.pose_information(cloud, pano, tr, ro)
        out[name + ".info.weighted"] = ops.pose_information(wcloud, pano, tr, ro)
        out[name + ".info.l1"] = ops.pose_information(cloud, pano, tr, ro, objective="l1")
        out[name + ".info.images"] = ops.pose_information_images(cloud, panos, tr[:2], ro[:2])
        out[name + ".info.images.l1"] = ops.pose_information_images(cloud, panos, tr[:2], ro[:2], objective="l1")
        out[name + ".gn"] = ops.gauss_newton_refine(cloud, pano, tr, ro, iters=3, trace=True)
        out[name + ".gn.l1"] = ops.gauss_newton_refine(cloud, pano, tr, ro, iters=3, trace=True, objective="l1")
        out[name + ".gn.images"] = ops.gauss_newton_refine_images(cloud, panos, tr[:2], ro[:2], iters=3, trace=True)
        out[name + ".gn.frozen"] = ops.gauss_newton_refine(cloud, pano, tr, ro, iters=3, trace=True, step_cap=1e-30)    # rows past the last evaluation
        if name != "S2":
            # rooms of different sizes in one frame x 2 images: R * I = 4 poses
            clouds = [cloud, ops.Cloud(X[:700].contiguous(), C[:700].contiguous())]
            t4, r4 = tr[[0, 1, 2, 0]].contiguous(), ro[[0, 1, 2, 0]].contiguous()
            out[name + ".info.rooms"] = ops.pose_information_rooms(clouds, panos, t4, r4)
            out[name + ".gn.rooms"] = ops.gauss_newton_refine_rooms(clouds, panos, t4, r4, iters=3, trace=True)
    return ws.flat(out)


@gpu
def test_information_and_polish(oracle):
    run("polish", lambda: polish(oracle))


# ------------------------------------------------------------------------------------------------- 4. the initialisation stage
NSH, NSW = 4, 4


def rot_table():
    """24 rotations in 6 (pitch, roll) classes of 4 yaws, one class at a pole"""
    rows = [(y, p, r) for p, r in ((0.0, 0.0), (0.4, 0.0), (0.0, -0.3), (np.pi / 2, 0.0), (-0.7, 0.2), (0.4, 0.5)) for y in (0.0, 1.5, 3.1, 4.7)]
    return np.array(rows, np.float32)


def init_stage(oracle):
    from piccolo_amd import ops
    out = {}
    for name in ("S1B4", "S1B3", "S2"):
        xyz, rgb, img, trans, rot = S(oracle, name)
        n, (H, W) = len(xyz), img.shape[:2]
        X, C, I, tr, ro = T(xyz), T(rgb), T(img), T(trans), T(rot)
        I2 = T(second_image(img))
        cloud = ops.Cloud(X, C)
        sets = ops.Cloud.with_color_sets(X, [C, C.flip(1).contiguous()], order=cloud.order)
        groups = ops.TrimGroups(T(rot_table()))
        out[name + ".ngroups"] = groups.ngroups
        for fmt in ("u8v", "u8p", "u8"):
            pano, pano2 = ops.Pano(I, fmt=fmt), ops.Pano(I2, fmt=fmt)
            order = ops.TrimOrder(cloud, pano.texels, tr, groups)
            k = "%s.%s." % (name, fmt)
            out[k + "table"] = ops.trim_loss_table(cloud, pano, tr, groups)
            out[k + "table.order"] = ops.trim_loss_table(cloud, pano, tr, groups, return_count=True, order=order)
            out[k + "tables"] = ops.trim_loss_tables(cloud, [pano, pano2], tr, groups, return_count=True, order=order)
            out[k + "tables.sets"] = ops.trim_loss_tables(sets, [pano, pano2], tr, groups, return_count=True)
        out[name + ".select"] = ops.select_poses(out[name + ".u8.table"].reshape(-1), 5, tr, T(rot_table()), rot_per_trans=24, return_idx=True)
        parts = ops.hist_trim_scores(I, cloud, tr, ro, NSH, NSW, return_parts=True)
        out[name + ".hist"] = parts
        out[name + ".hist.batch"] = ops.hist_trim_scores(I, cloud, tr, ro, NSH, NSW, batch=3, return_parts=True)
        out[name + ".hist.splat"] = ops.hist_trim_scores(I, cloud, tr, ro, NSH, NSW, return_parts=True, splat=True)
        ti, ri = torch.stack([tr, tr.flip(0)]).contiguous(), torch.stack([ro, ro.flip(0)]).contiguous()
        out[name + ".hist.images"] = ops.hist_trim_scores_images([I, I2], cloud, ti, ri, NSH, NSW)
        out[name + ".hist.images.splat"] = ops.hist_trim_scores_images([I, I2], cloud, ti, ri, NSH, NSW, splat=True)
        out[name + ".hist.sets"] = ops.hist_trim_scores_images([I, I2], sets, ti, ri, NSH, NSW)
        out[name + ".hist.sets.splat"] = ops.hist_trim_scores_images([I, I2], sets, ti, ri, NSH, NSW, splat=True)
        maps = ops.score_maps(cloud, tr, ro, H, W, NSH, NSW, parts[1], parts[2], parts[3])
        out[name + ".maps"] = maps
        packed = ops.score_maps(cloud, tr, ro, H, W, NSH, NSW, parts[1], parts[2], parts[3], packed=True)
        out[name + ".maps.packed"] = packed
        out[name + ".score.weights"] = ops.score_weight_plane(n, packed[0], packed[1], floor=0.25)
        out[name + ".box"] = ops.quantile_box(X, 0.05)
        cam = ops.transform_cloud(X, tr[0], ro[0])
        out[name + ".cam"] = cam
        out[name + ".pano"] = ops.make_pano(cam, C, (H, W))
        out[name + ".pano.odd"] = ops.make_pano(cam, C, (31, 63))
        out[name + ".zmin"] = ops.scatter_min_depth(cam, (H, W))
    return ws.flat(out)


def make_input():
    """utils.make_input end to end on the 5000-point configuration of the make_input golden (its inputs only: the init_dict, cloud and image)"""
    from conftest import load_golden
    from piccolo_amd import utils
    from test_oracle_golden import g23_case
    xyz, rgb, img, init, n_in, n_mid, _ = g23_case(load_golden("g23_make_input.npz"), "stanford_parallel")
    X, C, I = T(xyz), T(rgb), T(img)
    out = {"input": utils.make_input(I, X, C, n_in, init, "loss_histogram", n_mid)}
    out["scored"] = utils.make_input_scored(I, X, C, n_in, init, "loss_histogram", n_mid)
    out["images"] = utils.make_input_images([I, T(second_image(img))], X, C, n_in, init, "loss_histogram", n_mid)
    return ws.flat(out)


def hist_last_resort(oracle):
    from piccolo_amd import ops
    xyz, rgb, img, trans, rot = S(oracle, "S2")
    return ws.flat({"hist": ops.hist_trim_scores(T(img), ops.Cloud(T(xyz), T(rgb)), T(trans), T(rot), NSH, NSW, return_parts=True)})


def run_hist_last_resort(oracle):
    """not one candidate's point lists fit: the allocation ladder of ops._hist_workspace ends at the z-buffer splat's small workspace"""
    from piccolo_amd import _lib
    lib = _lib.load()
    splat, binned = lib.pcl_hist_trim_workspace_bytes(1, 64, 128, NSH, NSW), lib.pcl_hist_trim_workspace_bytes_n(50001, 1, 64, 128, NSH, NSW)
    assert 0 < splat < binned
    run("hist_last_resort", lambda: hist_last_resort(oracle), refuse_above=splat, refuse_in="_hist_workspace")


@gpu
def test_initialisation_stage(oracle):
    run("init_stage", lambda: init_stage(oracle))


@gpu
def test_make_input():
    run("make_input", make_input)


@gpu
def test_histogram_ladder_last_resort(oracle):
    run_hist_last_resort(oracle)
    assert ("bytes", ("_hist_workspace", [ln for f, ln in ws.bytes_sites() if f == "_hist_workspace"][-1])) in SEEN["hist_last_resort"]


# ------------------------------------------------------------------------------------------------- 5. colour
def colour(oracle):
    from piccolo_amd import color_utils, ops
    out = {}
    for name, im in (("S1", S(oracle, "S1B4")[2]), ("odd", img31(oracle)), ("S2", S(oracle, "S2")[2])):
        rgb = S(oracle, "S2" if name == "S2" else "S1B4")[1]
        I, C = T(im), T(rgb)
        out[name + ".template"] = ops.ColorTemplate(C).data
        out[name + ".match"] = color_utils.color_match(I, C)
        out[name + ".mod"] = color_utils.color_mod(I, C, 256)
        out[name + ".mod.17"] = ops.color_mod(I, C, num_bins=17)
        mask = (I.sum(-1) > 0.5)
        for ch in ((8, 8, 8), (17, 17, 17), (3, 5, 7)):          # 512 bins: counted in LDS; 4913: past PCL_HIST_LDS_BINS, in global memory
            h = ops.histogram(I, mask, ch)
            out[name + ".hist.%d" % ch[0]] = h
            out[name + ".hist.raw.%d" % ch[0]] = ops.histogram(I, mask, ch, normalize=False)
            h2 = ops.histogram(I.flip(1).contiguous(), torch.ones_like(mask), ch, eps=1e-6)
            out[name + ".inter.%d" % ch[0]] = ops.histogram_intersection(torch.stack([h, h2, h]), torch.stack([h2, h2, h]))
            out[name + ".hist.batch.%d" % ch[0]] = ops.histogram(torch.stack([I, I.flip(1)]), torch.stack([mask, torch.ones_like(mask)]), ch, eps=1e-6)
    return ws.flat(out)


@gpu
def test_colour(oracle):
    run("colour", lambda: colour(oracle))


# ------------------------------------------------------------------------------------------------- 6. GD chains
def finish(gd, hist=None):
    return {"history": hist, "result": gd.result(), "winner": gd.winner()}


def gd_chains(oracle):
    from piccolo_amd import ops
    out = {}
    for name in ("S1B4", "S1B3", "S2B66"):
        xyz, rgb, img, trans, rot = S(oracle, name)
        n, B = len(xyz), len(trans)
        X, C, I, tr, ro = T(xyz), T(rgb), T(img), T(trans), T(rot)
        cloud, pano = ops.Cloud(X, C), ops.Pano(I)
        pano2 = ops.Pano(T(second_image(img)))
        box = ops.quantile_box(X, 0.05)
        for mode in (True, False):
            gd = ops.GradientDescent(cloud, pano, tr, ro, box, batch_mode=mode)
            out["%s.plain.%d" % (name, mode)] = finish(gd, gd.run(7, history=True))
        gd = ops.GradientDescent(cloud, pano, tr, ro, box, fuse=False)
        out[name + ".two"] = finish(gd, gd.run(7, history=True))
        gd = ops.GradientDescent(ops.Cloud(X, C, order=cloud.order, weights=T(weights_of(n))), pano, tr, ro, box)
        out[name + ".weighted"] = finish(gd, gd.run(7, history=True))
        gd = ops.GradientDescent(cloud, pano, tr, ro, box)
        out[name + ".robust"] = finish(gd, gd.run_robust(7, [3], history=True))
        out[name + ".robust.plane"] = gd._robust["plane"]
        out[name + ".robust.scale"] = gd._robust["scale"]
        gd = ops.GradientDescent(cloud, pano, tr, ro, box, depth_mask=True)
        out[name + ".depth"] = finish(gd, gd.run(7, history=True))
        gd = ops.GradientDescent(cloud, pano, tr, ro, box)
        gd.run(3)
        leaf_t, leaf_r = torch.zeros(B, 3, device="cuda"), torch.zeros(B, 3, device="cuda")
        child, survivors = gd.pruned(2, leaf_t, leaf_r)
        out[name + ".pruned"] = dict(finish(child, child.run(4, history=True)), survivors=survivors, leaf_t=leaf_t, leaf_r=leaf_r)
        gd = ops.GradientDescent(cloud, pano, tr, ro, box)
        gd.run_graph(5)
        out[name + ".graph"] = finish(gd)
        if name != "S1B4":
            continue
        # two images of two candidates each: weight sets, colour sets, colour sets under the depth mask
        gd = ops.GradientDescent(cloud, pano, tr, ro, box, weight_sets=2)
        gd.set_pano_groups([pano, pano2])
        out[name + ".weight.sets"] = dict(finish(gd, gd.run_robust(7, [3], kind="huber", history=True)), planes=gd.weight_planes(), winners=gd.winner(2))
        sets = ops.Cloud.with_color_sets(X, [C, C.flip(1).contiguous()], order=cloud.order)
        for depth in (False, True):
            gd = ops.GradientDescent(sets, pano, tr, ro, box, depth_mask=depth)
            gd.set_pano_groups([pano, pano2])
            out["%s.colour.sets.%d" % (name, depth)] = dict(finish(gd, gd.run(7, history=True)), winners=gd.winner(2))
    return ws.flat(out)


def room_scene():
    """three rooms of different sizes side by side, two 32 x 64 images (of rooms 0 and 1), starts per (room, image)"""
    import room_helpers as rh
    rooms = rh.rooms((1025, 700, 301), seed=3)
    imgs = [rh.query(rooms, r, 40 + r, res=(32, 64))[0] for r in (0, 1)]
    return rooms, imgs, rh.image_starts(3, 2, 2, seed=5)


def gd_rooms():
    from piccolo_amd import ops
    out = {}
    rooms, imgs, st = room_scene()
    clouds = [ops.Cloud(x, c) for x, c in rooms]
    pairs = [(c, ops.quantile_box(x, 0.05)) for c, (x, _) in zip(clouds, rooms)]
    panos = [ops.Pano(im) for im in imgs]
    one_t, one_r = torch.cat([st[r][0][0] for r in range(3)]), torch.cat([st[r][0][1] for r in range(3)])
    gd = ops.GradientDescentRooms(pairs, panos[0], one_t, one_r)
    out["rooms"] = finish(gd, gd.run(7, history=True))
    gd = ops.GradientDescentRooms(pairs, panos[0], one_t, one_r, depth_mask=True, depth_tau=0.1)
    out["rooms.depth"] = finish(gd, gd.run(7, history=True))
    gd = ops.GradientDescentRooms(pairs, panos[0], one_t, one_r)
    gd.run(3)
    child, survivors = gd.pruned(1)
    out["rooms.pruned"] = dict(finish(child, child.run(4, history=True)), survivors=survivors)
    all_t = torch.cat([st[r][i][0] for r in range(2) for i in range(2)])
    all_r = torch.cat([st[r][i][1] for r in range(2) for i in range(2)])
    for depth in (False, True):
        gd = ops.GradientDescentRoomsImages(pairs[:2], panos, all_t, all_r, depth_mask=depth, depth_tau=0.1 if depth else None)
        out["rooms.images.%d" % depth] = finish(gd, gd.run(7, history=True))
    gd = ops.GradientDescentRoomsImages(pairs[:2], panos, all_t, all_r, batch_mode=False, fuse=False)
    out["rooms.images.sequential"] = finish(gd, gd.run(7, history=True))
    return ws.flat(out)


@gpu
def test_gd_chains(oracle):
    run("gd_chains", lambda: gd_chains(oracle))


@gpu
def test_gd_rooms_chains():
    run("gd_rooms", gd_rooms)


# ------------------------------------------------------------------------------------------------- 7. the front end
BASE = dict(num_iter=8, num_input=4, lr=0.1, patience=5, factor=0.9, out_of_room_quantile=0.05)


def front_end(oracle):
    from conftest import Cfg
    from piccolo_amd import omniloc as po
    out = {}
    xyz, rgb, img, trans, rot = S(oracle, "S1B4")
    X, C, I = T(xyz), T(rgb), T(img)
    I2 = T(second_image(img))
    for tag, kw in (("robust", dict(robust_iters=[3])), ("pruned", dict(prune_iters=[3], prune_keep=[2])), ("l1", dict(gn_objective="l1"))):
        t, r = T(trans), T(rot)
        got = po.omniloc_batch(I, X, C, t, r, Cfg(**BASE, gn_iters=2, pose_covariance=True, **kw), {})
        out["batch." + tag] = dict(got=got, leaf_t=t, leaf_r=r)
    t, r = T(trans), T(rot)
    out["batch.cov"] = dict(got=po.omniloc_batch(I, X, C, t, r, Cfg(**BASE, pose_covariance=True), {}, weights=T(weights_of(len(xyz)) + 0.25)), t=t, r=r)
    for tag, colours, kw in (("shared", C, {}), ("sets", [C, C.flip(1).contiguous()], {}), ("robust", C, dict(robust_iters=[3]))):
        tl, rl = [T(trans), T(trans[::-1])], [T(rot), T(rot[::-1])]
        got = po.omniloc_batch_images_polished([I, I2], X, colours, tl, rl, Cfg(**BASE, gn_iters=2, pose_covariance=True, **kw))
        out["images." + tag] = dict(got=got, leaf_t=tl, leaf_r=rl)
    return ws.flat(out)


def front_end_rooms():
    from conftest import Cfg
    from piccolo_amd import omniloc as po
    rooms, imgs, st = room_scene()
    tl = [[st[r][i][0].clone() for i in range(2)] for r in range(2)]
    rl = [[st[r][i][1].clone() for i in range(2)] for r in range(2)]
    got, chain_loss = po.omniloc_batch_rooms_images_polished(imgs, rooms[:2], tl, rl, Cfg(**dict(BASE, num_input=2), gn_iters=2, pose_covariance=True))
    return ws.flat(dict(got=got, chain_loss=chain_loss, leaf_t=tl, leaf_r=rl))


@gpu
def test_front_end(oracle):
    run("front_end", lambda: front_end(oracle))


@gpu
def test_front_end_rooms():
    run("front_end_rooms", front_end_rooms)


# ------------------------------------------------------------------------------------------------- the harness once more, on CUDA tensors
@gpu
def test_harness_guards_on_cuda():
    for where in (N_WS, -1):
        with pytest.raises(AssertionError, match=r"_overrun:\d+ \(64 bytes\) wrote at offset %d$" % where):
            _overrun("cuda", where)
    _overrun("cuda", N_WS - 1)


# ------------------------------------------------------------------------------------------------- census (the last test of the file)
SCENARIOS = {
    "packing": test_packing, "loss": test_loss, "polish": test_information_and_polish, "init_stage": test_initialisation_stage,
    "make_input": lambda oracle: test_make_input(), "hist_last_resort": run_hist_last_resort, "colour": test_colour, "gd_chains": test_gd_chains,
    "gd_rooms": lambda oracle: test_gd_rooms_chains(), "front_end": test_front_end, "front_end_rooms": lambda oracle: test_front_end_rooms(),
}


@gpu
def test_census(oracle):
    """every `_bytes(` call site of ops.py was reached by a scenario; a workspace added later fails here until one covers it"""
    for name, scenario in SCENARIOS.items():
        if name not in SEEN:
            scenario(oracle)
    sites = set(ws.bytes_sites())
    print("\n| site of ops.py | scenarios |\n|---|---|")
    for f, ln in sorted(sites, key=lambda s: s[1]):
        print("| %s:%d | %s |" % (f, ln, ", ".join(name for name, seen in SEEN.items() if ("bytes", (f, ln)) in seen) or "-"))
    reached = {c for seen in SEEN.values() for k, c in seen if k == "bytes"}
    assert reached - sites == set(), "recorded callers the walk does not know: %s" % sorted(reached - sites)
    assert sites - reached == set(ALLOWED), "call sites no scenario reached: %s" % sorted(sites - reached - set(ALLOWED))
