"""pcl_gd_run as two half-chains on two streams (pcl_gd_hyper.fuse -3: split whenever there are two pose groups, -2: never):
the split changes WHERE and WHEN the pose groups are evaluated, never what — every group runs under the whole chain's plan — so
result(), the loss history and the canonical copy of the optimiser state must agree BIT FOR BIT between the two forms.  Nothing here
depends on timing."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 64, 128
SPLIT, NEVER = -3, -2


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def scene(ops, oracle):
    """one 20 001-point box room (40 chunks of one 512-point step, the last one of 33 points), two panoramas, its clamp box"""
    s = make_scene(ops, oracle, 20_001, 41, 2)
    w = (0.25 + np.random.default_rng(7).random(s["n"])).astype(np.float32)
    s["weighted"] = ops.Cloud(s["X"], s["C"], weights=torch.from_numpy(w).cuda())
    return s


def make_scene(ops, oracle, n, seed, images):
    from piccolo_amd import synth
    xyz, rgb = synth.box_room(n, seed)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    panos, gts = [], []
    for k in range(images):
        t_gt, ypr_gt = synth.gt_pose(seed + k)
        img = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb, (H, W)).astype(np.float32) / 255
        panos.append(ops.Pano(torch.from_numpy(img).cuda()))
        gts.append((t_gt, ypr_gt))
    return {"n": n, "X": X, "C": C, "cloud": ops.Cloud(X, C), "box": ops.quantile_box(X, 0.05), "panos": panos, "gts": gts}


def starts(scene, B, image=0):
    from piccolo_amd import synth
    tr, ro = synth.start_poses(*scene["gts"][image], B, seed=300 + B + image)
    tr[0, 0] = 4.4                                             # one start outside the clamp box (batch mode's clamp lag)
    return torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()


def engine(ops, scene, B, fuse, batch_mode=True, table=None, cloud="cloud"):
    tr, ro = starts(scene, B)
    gd = ops.GradientDescent(scene[cloud], scene["panos"][0], tr, ro, scene["box"], lr=0.1, patience=5, factor=0.8, batch_mode=batch_mode, fuse=fuse)
    if table is not None:
        gd.set_panos([scene["panos"][i] for i in table])
    return gd


def outcome(gd, hist):
    """what a caller can see, and the canonical copy of the state blob (B x (160 B state + 64 B pose record)) byte for byte"""
    return hist.clone(), gd.result().clone(), gd.state.clone()[: gd.B * (160 + 64)]


def same(a, b, what):
    for x, y, name in zip(a, b, ("loss history", "result", "optimiser state")):
        assert x.shape == y.shape and torch.equal(x, y), (what, name)


def plan(ops, n, B, fuse):
    nch, G, fz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    hy = ops._gd_hyper(0.1, 5, 0.8, True, fuse)
    assert ops._lib.load().pcl_gd_plan_hyper(n, B, ctypes.byref(hy), ctypes.byref(nch), ctypes.byref(G), ctypes.byref(fz)) == 0
    return nch.value, G.value, fz.value


def test_the_switch_reaches_the_struct(ops):
    assert [ops._gd_hyper(0.1, 5, 0.8, True, f).fuse for f in (None, True, False, 0, -1, -2, -3)] == [0, 0, -1, 0, -1, -2, -3]
    with pytest.raises(ValueError):
        ops._gd_hyper(0.1, 5, 0.8, True, -4)
    # -2 and -3 are two-launch forms like -1: never fused
    assert plan(ops, 20_001, 8, NEVER)[2] == 0 and plan(ops, 20_001, 8, SPLIT)[2] == 0


@pytest.mark.parametrize("B, batch_mode", [(8, True), (8, False), (6, True), (3, True)])
def test_split_equals_single_stream(ops, scene, B, batch_mode):
    """B = 8: four groups, 2 + 2 (A's first launch goes out as 1 + 1), batch and sequential mode; B = 6: three groups, 1 + 2; B = 3: one
    pose per block, three groups"""
    nch, G, _ = plan(ops, scene["n"], B, SPLIT)
    assert G == (2 if B % 2 == 0 else 1) and B // G >= 2
    out = {}
    for fuse in (SPLIT, NEVER):
        gd = engine(ops, scene, B, fuse, batch_mode)
        out[fuse] = outcome(gd, gd.run(12, history=True))
    same(out[SPLIT], out[NEVER], (B, batch_mode))
    assert torch.isfinite(out[SPLIT][0]).all()


@pytest.mark.parametrize("table", [[0] * 4 + [1] * 4, [0] * 2 + [1] * 6, [0] * 6 + [1] * 2])
def test_two_images_with_a_panorama_table(ops, scene, table):
    """B = 2 x 4 and uneven tables: the split (after group 2 of 4, pose 4) falls between the images or inside one of them"""
    out = {}
    for fuse in (SPLIT, NEVER):
        gd = engine(ops, scene, 8, fuse, table=table)
        out[fuse] = outcome(gd, gd.run(12, history=True))
    same(out[SPLIT], out[NEVER], table)
    # (the two images do differ: the table is not ignored)
    assert not torch.equal(out[SPLIT][0][:, 0], out[SPLIT][0][:, 7])


def test_weighted_cloud(ops, scene):
    out = {}
    for fuse in (SPLIT, NEVER):
        gd = engine(ops, scene, 4, fuse, cloud="weighted")
        out[fuse] = outcome(gd, gd.run(12, history=True))
    same(out[SPLIT], out[NEVER], "weighted")
    plain = engine(ops, scene, 4, NEVER)
    assert not torch.equal(plain.run(12, history=True), out[NEVER][0])             # (the weights are not ignored)


def test_short_runs_and_runs_in_pieces(ops, scene):
    """0, 1 and 2 iterations (the stagger lives in the first one), and 5 + 7 iterations continuing one another like 12 in one call"""
    for num_iter in (0, 1, 2):
        out = {}
        for fuse in (SPLIT, NEVER):
            gd = engine(ops, scene, 8, fuse)
            out[fuse] = outcome(gd, gd.run(num_iter, history=True))
        same(out[SPLIT], out[NEVER], num_iter)
    whole = engine(ops, scene, 8, NEVER)
    ref = outcome(whole, whole.run(12, history=True))
    gd = engine(ops, scene, 8, SPLIT)
    pieces = torch.cat([gd.run(5, history=True), gd.run(7, history=True)])
    same(outcome(gd, pieces), ref, "5 + 7")


def test_caller_stream_sees_the_finished_state(ops, scene):
    """run() on a non-default stream, result() enqueued right behind it with no synchronisation in between: the join orders B's half
    before whatever the caller enqueues next"""
    ref_gd = engine(ops, scene, 8, NEVER)
    ref = outcome(ref_gd, ref_gd.run(12, history=True))
    gd = engine(ops, scene, 8, SPLIT)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        hist = gd.run(12, history=True)
        res = gd.result()
    st.synchronize()
    assert torch.equal(res, ref[1]) and torch.equal(hist, ref[0])


def test_the_rule_splits_large_chains_and_graphs_stay_unsplit(ops, oracle):
    """40 000 points x 128 candidates: 32 chunks x 64 groups = 2048 loss blocks, two halves of one full residency each — a size at
    which fuse = 0 / -1 split on their own (from 896 blocks per half).  Eager (split by the rule) and run_graph (a capturing caller
    keeps the one-stream chain) must both equal fuse = -2."""
    n, B = 40_000, 128
    nch, G, fz = plan(ops, n, B, None)
    assert fz == 0 and (B // G // 2) * nch >= 1024, (nch, G, fz)
    big = make_scene(ops, oracle, n, 43, 1)

    def make(fuse):
        return engine(ops, big, B, fuse)

    never = make(NEVER)
    ref = outcome(never, never.run(12, history=True))
    for fuse in (None, False):
        eager = make(fuse)
        same(outcome(eager, eager.run(12, history=True)), ref, ("eager", fuse))
    graph = make(None)
    graph.run_graph(12)
    assert torch.equal(graph.result(), ref[1]) and torch.equal(graph.state[: B * (160 + 64)], ref[2])
    graph.run_graph(12)                                         # (a replay continues the state: 24 iterations)
    never.run(12)
    assert torch.equal(graph.result(), never.result())


def test_fused_shapes_are_unchanged(ops, scene):
    """fuse = 0 at a shape whose blocks are all resident at once still runs one launch per iteration and still equals fuse = -1"""
    assert plan(ops, scene["n"], 8, None)[2] == 1
    out = {}
    for fuse in (None, False):
        gd = engine(ops, scene, 8, fuse)
        out[fuse] = outcome(gd, gd.run(12, history=True))
    same(out[None], out[False], "fused")
