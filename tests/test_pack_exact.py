"""The packers (csrc/pcl_pack.hip) word for word against the integer models of tests/ops_models.py.

The rule: what a packer writes is a pure re-arrangement of its input, so the whole buffer — every texel, plane, pad word and border — is
built by a numpy model from the layout rules of include/piccolo_hip.h and compared BIT FOR BIT; nothing here has a tolerance.  Buffers
handed to the C ABI are filled with a poison byte first, so a word the packer skips cannot equal the model by luck.

Panorama: five texel layouts (f32, u8, f16, u8p, u8v) over every combination of H in {1, 2, 3, 8} and W in {1, 2, 5, 32}: odd and even
  H + 2 for the row-pair interleave (the dangling half pair is zero), the last row's lower texel of the vertical pairs, the fp16 levels.
not_exact: the 256 levels and -0.0 are exact; the fp32 neighbours of k/255, -1/255, 256/255, inf and NaN are not, whether they sit in the
  first pixel or in the last channel of the last one.
Cloud: planes xyz[order] and -rgb[order] with +0.0 padding; colour sets across more than one launch (16 sets each) equal the single-set
  packs plane by plane; the weights plane, its refusals, and the all-zero plane after a refusal.
Morton order: lattice coordinates k 2^-10 make every key an exact integer, so the order EQUALS numpy's stable argsort of the keys — also with
  the bounding box's extremes beyond the first trip of its grid-stride loop (262 144 points), and with an axis of zero extent.
The CPU part plants layout mistakes into the models; each must change the bytes that are compared."""
import ctypes

import numpy as np
import pytest

import ops_models as om

gpu = pytest.mark.gpu
F32 = np.float32
HS, WS = (1, 2, 3, 8), (1, 2, 5, 32)
LEVEL_FMTS = ("u8", "f16", "u8p", "u8v")
CODE = {"f32": 0, "u8": 1, "f16": 2, "u8p": 3, "u8v": 4}
POISON = 0xA5


def _levels(H, W):
    rng = np.random.default_rng(100 * H + W)
    lv = rng.integers(0, 256, (H, W, 3))
    lv[0, 0], lv[-1, -1] = (255, 0, 1), (2, 254, 255)
    return lv


def _morton_cloud(kind):
    """lattice clouds (om.lattice) with both extremes on every axis, duplicated rows among them"""
    top = om.MORTON_TOP
    if kind == "one":
        return om.lattice(np.array([[5, 77, top]]))
    rng = np.random.default_rng(len(kind))
    if kind == "tail":                                # 262 144 interior points, the extremes among the 257 that follow
        k = np.concatenate([rng.integers(2 ** 19, 2 ** 20, (262144, 3)), rng.integers(0, top + 1, (257, 3))])
        k[262144 + 5], k[262144 + 250] = 0, top
        k[1000:1010], k[262144 + 100:262144 + 104] = k[7], k[262144 + 9]
        k[262144 + 200] = k[3]                        # a tail point equal to a head point: the head one stays in front
    else:
        k = rng.integers(0, top + 1, (257, 3))
        k[40], k[200] = 0, top
        k[10:16], k[256] = k[3], k[100]
        if kind == "flat":
            k[:, 2] = 12345                           # hi == lo: the axis contributes no key bits
    return om.lattice(k)


# ===================================================================================================== the models themselves (CPU)
def test_pano_models_have_the_padded_sizes():
    for H in HS:
        for W in WS:
            lv = _levels(H, W)
            for fmt in om.PANO_FMTS:
                assert len(om.pack_pano(lv, fmt)) == om.pano_bytes(H, W, fmt)
            p = om.pack_pano(lv, "u8p").view(np.uint32).reshape((H + 3) >> 1, W + 2, 2)
            if (H + 2) % 2:
                assert (p[-1] == 0).all()                           # the lower border row and the dangling half pair next to it
            assert p[(H >> 1), 1:-1, H & 1].any()                   # the image's last row, in the pair and half its parity says
            u8 = om.pack_pano(lv, "u8").view(np.uint32).reshape(H + 2, W + 2)
            assert (u8[0] == 0).all() and (u8[-1] == 0).all() and (u8[:, 0] == 0).all() and (u8[:, -1] == 0).all() and (u8 >> 24 == 0).all()


def test_planted_layout_mistakes_change_the_bytes():
    for H in HS:
        for W in WS:
            lv = _levels(H, W)
            assert not np.array_equal(om.pack_pano(lv, "u8p", swap_parity=True), om.pack_pano(lv, "u8p")), (H, W)
            assert not np.array_equal(om.pack_pano(lv, "u8v", shift_lower=True), om.pack_pano(lv, "u8v")), (H, W)


def test_planted_colour_set_launch_mistake_changes_the_planes():
    rng = np.random.default_rng(1)
    xyz = rng.normal(size=(257, 3)).astype(F32)
    for nsets in (1, 2, 16, 17, 33):
        rgbs = [rng.uniform(0, 1, (257, 3)).astype(F32) for _ in range(nsets)]
        same = np.array_equal(om.bits(om.pack_cloud_sets(xyz, rgbs, second_launch_at_0=True)), om.bits(om.pack_cloud_sets(xyz, rgbs)))
        assert same == (nsets <= 16)


def test_lattice_keys_are_exact_and_a_short_bounding_box_shows():
    for kind in ("one", "n257", "flat", "tail"):
        xyz = _morton_cloud(kind)
        k = np.rint(xyz.astype(np.float64) * 1024).astype(np.uint64)
        assert np.array_equal(k.astype(np.float64) / 1024, xyz.astype(np.float64))
        if kind in ("n257", "tail"):                  # fp32 quantisation = the integers themselves
            exact = om._spread21(k[:, 0]) | (om._spread21(k[:, 1]) << np.uint64(1)) | (om._spread21(k[:, 2]) << np.uint64(2))
            assert np.array_equal(om.morton_keys(xyz), exact)
            assert len(np.unique(exact)) < len(exact)                                                     # equal keys: stability matters
    xyz = _morton_cloud("tail")
    assert not np.array_equal(om.morton_order(xyz, box_rows=262144), om.morton_order(xyz))
    assert np.array_equal(om.morton_keys(_morton_cloud("flat")) & np.uint64(0x4924924924924924), np.zeros(257, np.uint64))


# ===================================================================================================== the device
@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned(nbytes):
    import torch
    return torch.full((int(nbytes),), POISON, dtype=torch.uint8, device="cuda")


def _pack_pano(ops, img, fmt):
    """-> (the packed buffer's bytes, the not_exact flag) through the C ABI"""
    import torch
    lib = ops._lib.load()
    H, W = img.shape[:2]
    nbytes = lib.pcl_pano_bytes(H, W, CODE[fmt])
    assert nbytes == om.pano_bytes(H, W, fmt)
    buf, flag, x = _poisoned(nbytes), torch.zeros(1, dtype=torch.int32, device="cuda"), T(img)        # (held until the copy back)
    if fmt == "f32":
        ops._lib.check(lib.pcl_pano_pack(ops._ptr(x), H, W, ops._ptr(buf), ops._stream()), "pcl_pano_pack")
    else:
        ops._lib.check(getattr(lib, "pcl_pano_pack_" + fmt)(ops._ptr(x), H, W, ops._ptr(buf), ops._ptr(flag), ops._stream()), fmt)
    return buf.cpu().numpy(), int(flag.item())


@gpu
@pytest.mark.parametrize("fmt", om.PANO_FMTS)
def test_pano_layouts_bit_for_bit(ops, fmt):
    for H in HS:
        for W in WS:
            lv = _levels(H, W)
            got, flag = _pack_pano(ops, om.levels_image(lv), fmt)
            assert flag == 0 and np.array_equal(got, om.pack_pano(lv, fmt)), (fmt, H, W)


@gpu
@pytest.mark.parametrize("fmt", LEVEL_FMTS)
def test_not_exact_flag(ops, fmt):
    H, W = 8, 32
    lv = (np.arange(H * W * 3) % 256).reshape(H, W, 3)
    img = om.levels_image(lv)
    img[tuple(np.argwhere(lv == 0)[1])] = -0.0
    assert np.signbit(img).sum() == 1 and len(np.unique(lv)) == 256
    got, flag = _pack_pano(ops, img, fmt)
    assert flag == 0 and np.array_equal(got, om.pack_pano(lv, fmt))            # -0.0 is level 0, the word of +0.0
    one = F32(1)
    bad = [np.nextafter(F32(k) / F32(255), s) for k in (1, 127, 254) for s in (-one, one)]
    bad += [F32(-1) / F32(255), F32(256) / F32(255), F32(np.inf), F32(np.nan)]
    for h, w in ((H, W), (1, 1), (3, 5)):
        base = om.levels_image(_levels(h, w))
        assert _pack_pano(ops, base, fmt)[1] == 0
        for v in bad:
            for at in ((0, 0, 0), (h - 1, w - 1, 2)):
                img = base.copy()
                img[at] = v
                assert _pack_pano(ops, img, fmt)[1] == 1, (fmt, h, w, at, v)


@gpu
def test_pano_refuses_or_falls_back_on_an_inexact_image(ops):
    img = om.levels_image(_levels(3, 5))
    img[2, 4, 2] = np.nextafter(img[2, 4, 2], F32(2))
    for fmt in ("u8", "f16", "u8p", "u8v"):
        with pytest.raises(ValueError):
            ops.Pano(T(img), fmt=fmt)
    p = ops.Pano(T(img), fmt="auto")
    assert p.fmt == CODE["f32"]
    n = om.pano_bytes(3, 5, "f32")
    exp = np.zeros((5, 7, 4), F32)
    exp[1:4, 1:6, :3] = img
    assert np.array_equal(p.data[:n].cpu().numpy(), exp.view(np.uint8).reshape(-1))


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz, rgb = rng.normal(size=(n, 3)).astype(F32), rng.uniform(0, 1, (n, 3)).astype(F32)
    rgb[0, 0], rgb[n - 1, 2], xyz[n - 1, 1] = 0.0, 0.0, -0.0                   # -rgb = -0.0 there: told from the padding's +0.0
    return xyz, rgb, rng.permutation(n)


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_cloud_pack_planes_and_padding(ops, n):
    lib = ops._lib.load()
    xyz, rgb, perm = _cloud(n, n)
    stride = lib.pcl_cloud_stride(n)
    assert stride == om.cloud_stride(n) and lib.pcl_cloud_bytes(n) == 24 * stride
    X, C = T(xyz), T(rgb)
    for order in (None, perm):
        buf = _poisoned(24 * stride)
        o = None if order is None else T(order.astype(np.int64))
        ops._lib.check(lib.pcl_cloud_pack(ops._ptr(X), ops._ptr(C), ops._ptr(o), n, ops._ptr(buf), ops._stream()), "pcl_cloud_pack")
        got = buf.cpu().numpy().view(np.uint32).reshape(6, stride)
        assert np.array_equal(got, om.bits(om.pack_cloud_sets(xyz, [rgb], order)))
        assert (got[:, n:] == 0).all()                                         # +0.0 in every padding slot
        c = ops.Cloud(X, C, sort=False) if order is None else ops.Cloud(X, C, order=o)
        assert np.array_equal(c.data[:24 * stride].cpu().numpy().view(np.uint32).reshape(6, stride), got)


@gpu
@pytest.mark.parametrize("nsets", [1, 2, 16, 17, 33])
def test_colour_sets_across_launches(ops, nsets):
    lib = ops._lib.load()
    n = 257
    xyz, _, perm = _cloud(n, 50 + nsets)
    rng = np.random.default_rng(nsets)
    rgbs = [rng.uniform(0, 1, (n, 3)).astype(F32) for _ in range(nsets)]
    stride = om.cloud_stride(n)
    nbytes = lib.pcl_cloud_sets_bytes(n, nsets)
    assert nbytes == 4 * stride * (3 + 3 * nsets)
    X = T(xyz)
    for order in (None, perm):
        o = None if order is None else T(order.astype(np.int64))
        dev = [T(r) for r in rgbs]
        arr = (ctypes.c_void_p * nsets)(*[r.data_ptr() for r in dev])
        buf = _poisoned(nbytes)
        ops._lib.check(lib.pcl_cloud_pack_sets(ops._ptr(X), arr, nsets, ops._ptr(o), n, ops._ptr(buf), ops._stream()), "pcl_cloud_pack_sets")
        got = buf.cpu().numpy().view(np.uint32).reshape(3 + 3 * nsets, stride)
        assert np.array_equal(got, om.bits(om.pack_cloud_sets(xyz, rgbs, order)))
        sets = ops.Cloud.with_color_sets(X, dev, order=o, sort=False)
        assert sets.color_sets == nsets and np.array_equal(sets.data[:nbytes].cpu().numpy().view(np.uint32).reshape(-1, stride), got)
        for k in range(nsets):                                                 # every set is the single-colour pack, xyz planes included
            c = ops.Cloud(X, dev[k], sort=False) if order is None else ops.Cloud(X, dev[k], order=o)
            one = c.data[:24 * stride].cpu().numpy().view(np.uint32).reshape(6, stride)
            assert np.array_equal(one[:3], got[:3]) and np.array_equal(one[3:], got[3 + 3 * k:6 + 3 * k]), (nsets, k)


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_weights_plane(ops, n):
    import torch
    lib = ops._lib.load()
    xyz, rgb, perm = _cloud(n, 70 + n)
    rng = np.random.default_rng(n)
    w = rng.uniform(0, 2, n).astype(F32)
    w[0], w[n - 1] = 0.0, np.finfo(F32).max                                    # the ends of what is accepted
    stride = om.cloud_stride(n)
    assert lib.pcl_cloud_weights_bytes(n) == 4 * stride
    X, C, Wt = T(xyz), T(rgb), T(w)
    for order in (None, perm):
        o = None if order is None else T(order.astype(np.int64))
        plane, bad = _poisoned(4 * stride), torch.zeros(1, dtype=torch.int32, device="cuda")
        ops._lib.check(lib.pcl_cloud_pack_weights(ops._ptr(Wt), ops._ptr(o), n, ops._ptr(plane), ops._ptr(bad), ops._stream()), "weights")
        assert int(bad.item()) == 0
        assert np.array_equal(plane.cpu().numpy().view(np.uint32), om.bits(om.pack_weights(w, order)))
        c = ops.Cloud(X, C, sort=False, weights=Wt) if order is None else ops.Cloud(X, C, order=o, weights=Wt)
        assert np.array_equal(om.bits(c.weights.cpu().numpy()), om.bits(om.pack_weights(w, order)))
        for v in (-1e-30, -0.5, np.nan, np.inf, -np.inf):
            wb = w.copy()
            wb[n - 1] = v                                                      # at the last point
            with pytest.raises(ValueError):
                ops.Cloud(X, C, sort=False, weights=T(wb))
            with pytest.raises(ValueError):
                c.set_weights(T(wb))
            assert (c.weights.view(torch.int32) == 0).all()                    # a refused plane is all zero: no vote rather than a wrong one
            c.set_weights(Wt)
            assert np.array_equal(om.bits(c.weights.cpu().numpy()), om.bits(om.pack_weights(w, order)))


def _cloud_order(ops, xyz):
    import torch
    lib = ops._lib.load()
    n = len(xyz)
    nws = lib.pcl_cloud_order_workspace_bytes(n)
    X, ws, order = T(xyz), _poisoned(max(nws, 16)), torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ops._lib.check(lib.pcl_cloud_order(ops._ptr(X), n, ops._ptr(order), ops._ptr(ws), nws, ops._stream()), "pcl_cloud_order")
    return order.cpu().numpy()


@gpu
@pytest.mark.parametrize("kind", ["one", "n257", "flat", "tail"])
def test_morton_order_equals_the_stable_argsort(ops, kind):
    xyz = _morton_cloud(kind)
    assert len(xyz) == {"one": 1, "n257": 257, "flat": 257, "tail": 262144 + 257}[kind]
    order = _cloud_order(ops, xyz)
    ref = om.morton_order(xyz)
    assert np.array_equal(order, ref), (kind, np.nonzero(order != ref)[0][:8])
    if kind != "one":                                                           # the wrapper sorts the same way
        assert np.array_equal(ops.Cloud(T(xyz), T(np.zeros_like(xyz))).order.cpu().numpy(), ref)
