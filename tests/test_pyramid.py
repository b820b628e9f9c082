"""The panorama pyramid on the device (pcl_pano_pyramid, pcl_gd_plateau_reset, ops.PanoPyramid, GradientDescent.run_pyramid and the cfg keys
pyramid_iters / pyramid_reset): the kernel against the numpy model of its rule bit for bit, and the coarse-to-fine chain against a
composition of code that existed before it — plain engines over plainly packed level images, the optimiser state copied from one to the
next.  No accuracy is asserted anywhere: whether coarse levels help is tools/pyramid_bench.py's table."""
import ctypes

import numpy as np
import pytest
import torch

import pyramid_helpers as ph
from conftest import Cfg
from parity_helpers import T

pytestmark = pytest.mark.gpu

FMTS = ("f16", "u8", "f32")
# the smallest shapes at which tiling can go wrong: one block of one level; no multiple of anything but 2; two levels on a ragged tile;
# every level count on a tile and a half; several tiles either way with ragged edges; a coarsest level (17 x 33) that crosses any tile
SHAPES = [(2, 2, 1), (6, 10, 1), (12, 20, 2), (16, 32, 1), (16, 32, 2), (16, 32, 3), (16, 32, 4), (48, 80, 4), (80, 48, 4), (272, 528, 4)]
POSE_BYTES, REC_BYTES = 160, 64            # PclGdPose, PclPoseRec (csrc/pcl_device.h): the state is {poses[B], records[B]} x 2
BEST, NUM_BAD = slice(8, 16), slice(116, 120)


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


_MODELS = {}


def model(H, W, levels):
    """(the uint8 image, its model levels), computed once per shape"""
    if (H, W, levels) not in _MODELS:
        lv0 = ph.planted_image(H, W, levels, seed=7 * H + W)
        _MODELS[(H, W, levels)] = (lv0, ph.pyramid(lv0, levels))
    return _MODELS[(H, W, levels)]


def run_kernel(ops, img, H, W, levels, codes, poison):
    """pcl_pano_pyramid into buffers pre-filled with the 32-bit word `poison`, a guard of 256 bytes behind each -> (texels, images) on the CPU"""
    lib = ops._lib.load()
    arr = (ctypes.c_int * levels)(*codes)
    nbytes = lib.pcl_pano_pyramid_bytes(H, W, levels, arr)
    assert nbytes > 0 and nbytes % 256 == 0
    nimg = sum(3 * (H >> l) * (W >> l) for l in range(1, levels + 1))
    tex = torch.full(((nbytes + 256) // 4,), poison, dtype=torch.int32, device=img.device)
    out = torch.full((nimg + 64,), poison, dtype=torch.int32, device=img.device)
    flag = torch.zeros(1, dtype=torch.int32, device=img.device)
    ops._lib.check(lib.pcl_pano_pyramid(ops._ptr(img), H, W, levels, arr, ops._ptr(tex), ops._ptr(out), ops._ptr(flag), ops._stream()), "pcl_pano_pyramid")
    assert int(flag.item()) == 0
    tex, out = tex.cpu(), out.cpu()
    assert (tex[nbytes // 4:] == poison).all() and (out[nimg:] == poison).all()          # nothing behind the buffers was touched
    return tex[:nbytes // 4].view(torch.uint8), out[:nimg].view(torch.float32)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("H,W,levels", SHAPES)
def test_kernel_against_the_model_bit_for_bit(ops, H, W, levels, fmt):
    lib = ops._lib.load()
    lv0, want = model(H, W, levels)
    img = T(ph.as_float(lv0))
    code = ops._PYRAMID_FMTS[fmt]
    tex_a, img_a = run_kernel(ops, img, H, W, levels, [code] * levels, 0x5A5A5A5A)
    tex_b, img_b = run_kernel(ops, img, H, W, levels, [code] * levels, -0x5A5A5A5B)     # 0xA5A5A5A5
    # identical bytes from two different poisons: every byte was written
    assert torch.equal(tex_a, tex_b) and torch.equal(img_a.view(torch.int32), img_b.view(torch.int32))
    off = at = 0
    for l, lv in enumerate(want, 1):
        h, w = H >> l, W >> l
        assert lv.shape == (h, w, 3)
        f = ph.as_float(lv)
        got = img_a[at:at + 3 * h * w].view(h, w, 3)
        assert torch.equal(got.view(torch.int32), torch.from_numpy(f).view(torch.int32)), (l, "float image")
        at += 3 * h * w
        # the level's texels: what the pack kernel of this format writes for the model's float image, border included
        size = lib.pcl_pano_bytes(h, w, code)
        packed = ops.Pano(T(f), fmt=fmt)
        assert packed.fmt == code
        assert torch.equal(tex_a[off:off + size], packed.data[:size].cpu()), (l, fmt, "texels")
        end = (size + 255) // 256 * 256
        assert not tex_a[off + size:off + end].any(), (l, "padding")
        off += end
    assert off == tex_a.numel() and at == img_a.numel()


def test_mixed_formats_and_the_python_objects(ops):
    H, W, levels = 48, 80, 4
    lv0, want = model(H, W, levels)
    img = T(ph.as_float(lv0))
    fmts = ["u8", "f32", "f16", "u8"]
    pyr = ops.PanoPyramid(img, levels, fmts=fmts, images=True)
    assert pyr.levels == 4 and len(pyr.panos) == 5 and len(pyr.images) == 4
    p0 = ops.Pano(img)
    assert pyr.panos[0].texels == p0.texels and torch.equal(pyr.panos[0].data, p0.data)        # level 0 is today's Pano, bit for bit
    for l, (lv, f) in enumerate(zip(want, fmts), 1):
        p, packed = pyr.panos[l], ops.Pano(T(ph.as_float(lv)), fmt=f)
        assert p.texels == packed.texels == (H >> l, W >> l, ops._PYRAMID_FMTS[f])
        assert p.data.data_ptr() % 256 == 0
        assert torch.equal(p.data, packed.data[:p.data.numel()])
        assert same_bits(pyr.images[l - 1], T(ph.as_float(lv)))
    for got, lv in zip(ops.pano_pyramid(img, levels), want):
        assert same_bits(got, T(ph.as_float(lv)))
    from piccolo_amd import utils
    for got, lv in zip(utils.pano_pyramid(img, 2), want):
        assert same_bits(got, T(ph.as_float(lv)))
    # the default formats: f16 without a point count, refine_texels' with one
    assert [p.fmt for p in ops.PanoPyramid(img, 2).panos[1:]] == [ops._lib.PANO_F16] * 2
    assert [p.fmt for p in ops.PanoPyramid(img, 2, n=10).panos[1:]] == [ops._PYRAMID_FMTS[ops.refine_texels(10, H >> l, W >> l)] for l in (1, 2)]
    assert ops.refine_texels(10, H >> 1, W >> 1) == "u8" and ops.refine_texels(10 ** 6, H >> 1, W >> 1) == "f16"
    # a view that starts on an odd float: the 8-byte alignment of the source is the object's business
    flat = torch.zeros(3 * H * W + 1, dtype=torch.float32, device=img.device)
    flat[1:] = img.reshape(-1)
    odd = flat[1:].view(H, W, 3)
    assert odd.data_ptr() % 8 == 4
    assert same_bits(ops.PanoPyramid(odd, 1, images=True).images[0], T(ph.as_float(want[0])))


def test_inexact_and_refused_inputs(ops, monkeypatch):
    from piccolo_amd import synth
    lv0, want = model(16, 32, 4)
    good = ph.as_float(lv0)
    for y, x, c, v in ((5, 7, 1, np.float32(0.5)), (0, 0, 0, np.float32(1e-3)), (15, 31, 2, np.nextafter(np.float32(1.0), np.float32(2.0))),
                       (8, 8, 0, np.float32(-1 / 255)), (3, 30, 2, np.float32("nan"))):
        bad = good.copy()
        bad[y, x, c] = v
        with pytest.raises(ValueError, match="not exactly k/255"):
            ops.PanoPyramid(T(bad), 1)
        with pytest.raises(ValueError, match="not exactly k/255"):
            ops.pano_pyramid(T(bad), 4)
    # a tagged image is not waited for: the flag is never read (a forbidden .item() would raise here)
    tagged = synth.mark_levels(T(good))
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "item", lambda self: (_ for _ in ()).throw(AssertionError("the flag was read")))
        pyr = ops.PanoPyramid(tagged, 2, images=True)
    assert same_bits(pyr.images[1], T(ph.as_float(want[1])))
    # refused shapes and formats, on the host
    for H, W, levels in ((16, 32, 0), (16, 32, 5), (6, 10, 2), (12, 20, 3), (16, 24, 4)):
        with pytest.raises(ValueError):
            ops.PanoPyramid(torch.zeros(H, W, 3), levels)
    for fmts in ("u8p", ["f16"], ["f16", "u8v"], ["f16", "f16", "f16"]):
        with pytest.raises(ValueError, match="fmts"):
            ops.PanoPyramid(T(good), 2, fmts=fmts)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        ops.PanoPyramid(torch.zeros(16, 32), 1)


# ------------------------------------------------------------------------------------------------ the chain
N, PH, PW, ITERS, NUM_ITER = 1025, 64, 128, [3, 6], 9
_SCENE = {}


def scene(oracle):
    """computed once: xyz, the shared rgb, an rgb per image, two uint8 query images with their model levels, per image 4 starting poses"""
    if not _SCENE:
        from piccolo_amd import synth
        xyz, rgb0 = synth.box_room(N, seed=N % 89)
        imgs, starts = [], []
        for i in range(2):
            t_gt, ypr_gt = synth.gt_pose(N % 97 + 7 * i)
            lv0 = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb0, (PH, PW))
            imgs.append([lv0] + ph.pyramid(lv0, 2))
            starts.append(synth.start_poses(np.asarray(t_gt, np.float32), np.asarray(ypr_gt, np.float32), 4, seed=N + i))
        rng = np.random.default_rng(5)
        rgbs = []
        for i in range(2):
            rgb = rgb0.copy()
            hit = rng.random(N) < 0.2
            rgb[hit] = rng.random((int(hit.sum()), 3)).astype(np.float32)
            rgbs.append(rgb)
        # every level holds data and black: the loss's mask means something on each
        for lv in imgs[0]:
            assert lv.any() and not lv.any(axis=2).all()
        _SCENE.update(xyz=xyz, rgb=rgb0, rgbs=rgbs, imgs=imgs, starts=starts)
    return _SCENE


def level_imgs(s, i):
    return [T(ph.as_float(lv)) for lv in s["imgs"][i]]


def box_of(ops, s):
    return ops.quantile_box(T(s["xyz"]), 0.05)


def composed(ops, cloud, panos, tr, ro, box, reset=False, **kw):
    """The chain from code that existed before it: a plain engine per level over that level's plainly packed image, coarsest first, each
    taking over the state tensor of the one before -> (the last engine, the history rows of all nine iterations)"""
    prev, hists = None, []
    for pano, k in zip(panos, (3, 3, 3)):
        gd = ops.GradientDescent(cloud, pano, tr, ro, box, **kw)
        if prev is not None:
            gd.state.copy_(prev.state)
            if reset:
                ops._lib.check(ops._lib.load().pcl_gd_plateau_reset(ops._ptr(gd.state), gd.B, ops._stream()), "pcl_gd_plateau_reset")
        hists.append(gd.run(k, history=True))
        prev = gd
    return prev, torch.cat(hists)


@pytest.mark.parametrize("B", [4, 3])
@pytest.mark.parametrize("fuse", [None, False])
def test_chain_is_the_composition_of_plain_engines(ops, oracle, B, fuse):
    s = scene(oracle)
    f0, f1, f2 = level_imgs(s, 0)
    cloud, box = ops.Cloud(T(s["xyz"]), T(s["rgb"])), box_of(ops, s)
    tr, ro = T(s["starts"][0][0][:B]), T(s["starts"][0][1][:B])
    pyr = ops.PanoPyramid(f0, 2)
    plain = [ops.Pano(f2, fmt="f16"), ops.Pano(f1, fmt="f16"), ops.Pano(f0)]
    for reset in (False, True):
        ref, ref_hist = composed(ops, cloud, plain, tr, ro, box, reset=reset, fuse=fuse)
        gd = ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box, fuse=fuse)
        hist = gd.run_pyramid([pyr], NUM_ITER, ITERS, reset_plateau=reset, history=True)
        assert hist.shape == (NUM_ITER, B) and same_bits(hist, ref_hist), (reset, "history")
        assert same_bits(gd.result(), ref.result()) and same_bits(gd.winner(), ref.winner()), reset
        assert torch.isfinite(hist).all() and (hist > 0).all()
        # the replayed form: a graph per segment, no history
        g = ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box, fuse=fuse)
        assert g.run_pyramid([pyr], NUM_ITER, ITERS, reset_plateau=reset, graph=True) is None
        assert same_bits(g.result(), ref.result()) and same_bits(g.winner(), ref.winner()), (reset, "graph")
        assert len(g._graphs) == 3 and len({k[-3:] for k in g._graphs}) == 3              # one graph per level's (H, W, fmt)
        # ... and once more on the same engine, from the start: the captured graphs are replayed, the bits are the same
        g.reset(tr, ro)
        g.run_pyramid([pyr], NUM_ITER, ITERS, reset_plateau=reset, graph=True)
        assert same_bits(g.result(), ref.result()) and len(g._graphs) == 3
    # one coarse level of a deeper pyramid: level 1, then the image
    ref, ref_hist = None, []
    for pano, k in ((plain[1], 4), (plain[2], 5)):
        e = ops.GradientDescent(cloud, pano, tr, ro, box, fuse=fuse)
        if ref is not None:
            e.state.copy_(ref.state)
        ref_hist.append(e.run(k, history=True))
        ref = e
    gd = ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box, fuse=fuse)
    assert same_bits(gd.run_pyramid([pyr], NUM_ITER, [4], history=True), torch.cat(ref_hist)) and same_bits(gd.result(), ref.result())


def test_level_formats_give_the_same_chain(ops, oracle):
    s = scene(oracle)
    f0 = level_imgs(s, 0)[0]
    cloud, box = ops.Cloud(T(s["xyz"]), T(s["rgb"])), box_of(ops, s)
    tr, ro = T(s["starts"][0][0]), T(s["starts"][0][1])
    out = []
    for fmts in ("f16", "u8", ["u8", "f16"], ["f16", "u8"]):          # (the two level formats: float4 texels interpolate k/255, other roundings)
        pyr = ops.PanoPyramid(f0, 2, fmts=fmts)
        gd = ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box)
        out.append((gd.run_pyramid([pyr], NUM_ITER, ITERS, history=True), gd.result()))
    for h, r in out[1:]:
        assert same_bits(h, out[0][0]) and same_bits(r, out[0][1])


def test_plateau_reset_touches_best_and_num_bad_alone(ops, oracle):
    s = scene(oracle)
    f0 = level_imgs(s, 0)[0]
    cloud, box, B = ops.Cloud(T(s["xyz"]), T(s["rgb"])), box_of(ops, s), 4
    tr, ro = T(s["starts"][0][0]), T(s["starts"][0][1])
    fresh = ops.GradientDescent(cloud, ops.Pano(f0), tr, ro, box).state.cpu()
    for fuse in (None, False):
        gd = ops.GradientDescent(cloud, ops.Pano(f0), tr, ro, box, fuse=fuse)
        gd.run(5)
        before = gd.state.cpu().clone()
        assert before.numel() == 2 * B * (POSE_BYTES + REC_BYTES)
        ops._lib.check(ops._lib.load().pcl_gd_plateau_reset(ops._ptr(gd.state), B, ops._stream()), "pcl_gd_plateau_reset")
        after = gd.state.cpu()
        touched = torch.zeros_like(before, dtype=torch.bool)
        for copy in range(2):
            for b in range(B):
                base = copy * B * (POSE_BYTES + REC_BYTES) + b * POSE_BYTES
                for field in (BEST, NUM_BAD):
                    touched[base + field.start:base + field.stop] = True
                    # what pcl_gd_init wrote into a fresh state's canonical copy (+inf, 0)
                    want = fresh[b * POSE_BYTES + field.start:b * POSE_BYTES + field.stop]
                    assert torch.equal(after[base + field.start:base + field.stop], want), (copy, b, field)
        assert torch.equal(after[~touched], before[~touched])
        # the run had moved `best` of the canonical copy
        best = before[:B * POSE_BYTES].view(B, POSE_BYTES)[:, BEST].contiguous().view(torch.float64)
        assert torch.isfinite(best).all()
        r = gd.result()
        assert torch.isinf(r[:, 15]).all() and (r[:, 14] == 0).all()
    inf = fresh[:POSE_BYTES][BEST].view(torch.float64)
    assert torch.isinf(inf).all() and (inf > 0).all() and not fresh[:POSE_BYTES][NUM_BAD].any()


@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_images_of_one_chain_are_their_own_chains(ops, oracle, colours):
    s = scene(oracle)
    box, x = box_of(ops, s), T(s["xyz"])
    if colours == "shared":
        cloud = ops.Cloud(x, T(s["rgb"]))
        singles = [cloud, cloud]
    else:
        singles = [ops.Cloud(x, T(r)) for r in s["rgbs"]]
        cloud = ops.Cloud.with_color_sets(x, [T(r) for r in s["rgbs"]], order=singles[0].order)
    pyrs = [ops.PanoPyramid(level_imgs(s, i)[0], 2) for i in range(2)]
    starts = [(T(tr[:3]), T(ro[:3])) for tr, ro in s["starts"]]
    multi = ops.GradientDescent(cloud, pyrs[0].panos[0], torch.cat([t for t, _ in starts]), torch.cat([r for _, r in starts]), box)
    hist = multi.run_pyramid(pyrs, NUM_ITER, ITERS, history=True)
    res, wins = multi.result(), multi.winner(2)
    for i in range(2):
        one = ops.GradientDescent(singles[i], pyrs[i].panos[0], *starts[i], box)
        h = one.run_pyramid([pyrs[i]], NUM_ITER, ITERS, history=True)
        assert same_bits(hist[:, 3 * i:3 * i + 3], h), (colours, i)
        assert same_bits(res[3 * i:3 * i + 3], one.result()) and same_bits(wins[i:i + 1], one.winner())
    # the two images are different problems
    assert not same_bits(hist[:, :3], hist[:, 3:])


def test_what_run_pyramid_refuses(ops, oracle):
    s = scene(oracle)
    f0 = level_imgs(s, 0)[0]
    x, box = T(s["xyz"]), box_of(ops, s)
    cloud = ops.Cloud(x, T(s["rgb"]))
    tr, ro = T(s["starts"][0][0]), T(s["starts"][0][1])
    pyr, small = ops.PanoPyramid(f0, 2), ops.PanoPyramid(T(ph.as_float(s["imgs"][0][1])), 2)
    gd = ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box)
    for iters in ([], [0], [9], [3, 3], [6, 3], [10]):
        with pytest.raises(ValueError, match="strictly increasing"):
            gd.run_pyramid([pyr], NUM_ITER, iters)
    with pytest.raises(ValueError, match="at least 3 coarse levels"):
        gd.run_pyramid([pyr], NUM_ITER, [2, 4, 6])
    with pytest.raises(ValueError, match="share sizes and texel formats"):
        gd.run_pyramid([pyr, small], NUM_ITER, ITERS)
    with pytest.raises(ValueError, match="share sizes and texel formats"):
        gd.run_pyramid([pyr, ops.PanoPyramid(f0, 2, fmts="u8")], NUM_ITER, ITERS)
    with pytest.raises(ValueError, match="3 pyramids for 4 candidates"):
        gd.run_pyramid([pyr] * 3, NUM_ITER, ITERS)
    masked = ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box)
    masked.hyper.depth_mask = 1                      # (the flag run_pyramid looks at; such an engine never runs here)
    with pytest.raises(ValueError, match="no depth mask"):
        masked.run_pyramid([pyr], NUM_ITER, ITERS)
    with pytest.raises(ValueError, match="without weight_sets"):
        ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box, weight_sets=2).run_pyramid([pyr] * 2, NUM_ITER, ITERS)
    with pytest.raises(ValueError, match="without weights"):
        ops.GradientDescent(ops.Cloud(x, T(s["rgb"]), weights=torch.ones(N)), pyr.panos[0], tr, ro, box).run_pyramid([pyr], NUM_ITER, ITERS)
    # nothing ran: the state is the initial one
    assert same_bits(gd.result(), ops.GradientDescent(cloud, pyr.panos[0], tr, ro, box).result())


# ------------------------------------------------------------------------------------------------ the front end
def front_reference(ops, s, i, rgb, B, reset=False):
    """the composition for image i as omniloc_batch packs it: the Morton-ordered cloud, refine_texels' formats level by level"""
    f0, f1, f2 = level_imgs(s, i)
    cloud = ops.Cloud(T(s["xyz"]), T(rgb))
    panos = [ops.Pano(f, fmt=ops.refine_texels(N, f.shape[0], f.shape[1])) for f in (f2, f1, f0)]
    tr, ro = T(s["starts"][i][0][:B]), T(s["starts"][i][1][:B])
    return composed(ops, cloud, panos, tr, ro, box_of(ops, s), reset=reset)[0], cloud, panos[2]


def entry_bits(entry, row):
    t, R, loss = entry[:3]
    return (same_bits(t.reshape(3), row[0:3].cpu()) and same_bits(R.reshape(9), row[3:12].cpu()) and same_bits(loss.reshape(1), row[12:13].cpu()))


@pytest.mark.parametrize("reset", [False, True])
def test_omniloc_batch_with_the_keys_is_the_composition(ops, oracle, reset):
    from piccolo_amd import omniloc
    s = scene(oracle)
    xyz, rgb, img = T(s["xyz"]), T(s["rgb"]), level_imgs(s, 0)[0]
    ref, cloud, pano0 = front_reference(ops, s, 0, s["rgb"], 4, reset)
    win = ref.winner()
    for graph in (True, False):
        cfg = Cfg(num_input=4, num_iter=NUM_ITER, pyramid_iters=ITERS, pyramid_reset=reset, gd_graph=graph)
        tr, ro = T(s["starts"][0][0]).clone(), T(s["starts"][0][1]).clone()
        got = omniloc.omniloc_batch(img, xyz, rgb, tr, ro, cfg, None)
        assert len(got) == 3 and entry_bits(got, win[0]), (reset, graph)
        assert same_bits(tr, ref.result()[:, 6:9]) and same_bits(ro, ref.result()[:, 9:12])       # the leaves are written back
        # a second call meets the cached engine and its graphs
        tr, ro = T(s["starts"][0][0]).clone(), T(s["starts"][0][1]).clone()
        assert entry_bits(omniloc.omniloc_batch(img, xyz, rgb, tr, ro, cfg, None), win[0])
    # without the keys the same call is the plain chain's: another result, and no pyramid engine in its way
    plain = omniloc.omniloc_batch(img, xyz, rgb, T(s["starts"][0][0]).clone(), T(s["starts"][0][1]).clone(), Cfg(num_input=4, num_iter=NUM_ITER), None)
    e = ops.GradientDescent(cloud, pano0, T(s["starts"][0][0]), T(s["starts"][0][1]), box_of(ops, s))
    e.run(NUM_ITER)
    assert entry_bits(plain, e.winner()[0]) and not entry_bits(plain, win[0])
    # with the gn keys: the polish of THAT winner, at level 0
    cfg = Cfg(num_input=4, num_iter=NUM_ITER, pyramid_iters=ITERS, pyramid_reset=reset, gn_iters=4, pose_covariance=True)
    got = omniloc.omniloc_batch(img, xyz, rgb, T(s["starts"][0][0]).clone(), T(s["starts"][0][1]).clone(), cfg, None)
    res = ops.gauss_newton_refine_at_winners(cloud, pano0, win, iters=4)
    took = bool(((res["accepted"] > 1) & ((res["status"] == 0) | (res["status"] == 3))).item())
    if took:
        loss = ops.sampling_loss(cloud, pano0, res["trans"], res["rot"], with_grad=False)[:, 0:1]
        row = torch.cat([res["trans"], ops.rot_from_ypr(res["rot"]).reshape(1, 9), loss], dim=1)[0]
    else:
        row = win[0]
    assert len(got) == 4 and entry_bits(got, row) and same_bits(got[3], res["cov"][0].cpu())


@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_omniloc_batch_images_with_the_keys_is_the_composition(ops, oracle, colours):
    from piccolo_amd import omniloc
    s = scene(oracle)
    xyz = T(s["xyz"])
    rgbs = [s["rgb"], s["rgb"]] if colours == "shared" else s["rgbs"]
    rgb = T(s["rgb"]) if colours == "shared" else [T(r) for r in rgbs]
    imgs = [level_imgs(s, i)[0] for i in range(2)]
    cfg = Cfg(num_input=3, num_iter=NUM_ITER, pyramid_iters=ITERS)
    trs, ros = [T(s["starts"][i][0][:3]).clone() for i in range(2)], [T(s["starts"][i][1][:3]).clone() for i in range(2)]
    got = omniloc.omniloc_batch_images(imgs, xyz, rgb, trs, ros, cfg)
    for i in range(2):
        ref = front_reference(ops, s, i, rgbs[i], 3)[0]
        assert entry_bits(got[i], ref.winner()[0]), (colours, i)
        assert same_bits(trs[i], ref.result()[:, 6:9]) and same_bits(ros[i], ref.result()[:, 9:12])
        # ... which is image i's own omniloc_batch run under the keys
        own = omniloc.omniloc_batch(imgs[i], xyz, T(rgbs[i]), T(s["starts"][i][0][:3]).clone(), T(s["starts"][i][1][:3]).clone(), cfg, None)
        assert all(same_bits(a, b) for a, b in zip(own, got[i]))
