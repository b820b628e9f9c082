"""Torch-tensor front end of the C ABI: device memory and streams come from PyTorch-ROCm (plumbing), every
computation is a HIP kernel in libpiccolo_hip.so.

Inputs may live on the CPU (the reference's harness hands over whatever `device` it picked, localize.py:124):
they are uploaded to cuda:0.  Without a GPU or without the library every call raises — there is no fallback.
"""
import ctypes

import torch

from . import _lib


class _Experiment:
    """A/B switches of the measured-and-rejected log (profiles/EXPERIMENTS.md).  The product reads NO environment variable: these are
    plain attributes, all None / False by default, set by a tool or a test in its own process (tools/_knobs.py maps the old PCL_*
    variables onto them for the sweep scripts).
      pano_fmt      "f16" | "f32": what Pano(fmt="auto") tries first / forces for the refinement's panorama
      trim_fmt      "u8" | "u8p" | "u8v": the trim launch's texel layout instead of ops.trim_texels' choice
      gd_graph      True | False: hipGraph replay of the refinement chain on / off whatever the problem size
      verify_levels True: ignore synth.mark_levels' tag (the device-side k/255 check is read back as for any tensor)"""
    pano_fmt = None
    trim_fmt = None
    gd_graph = None
    verify_levels = False


EXPERIMENT = _Experiment()

F32 = torch.float32


_GPU_SEEN = False        # torch.cuda.is_available() answered True once (it is re-asked until then: the product must fail loudly without a GPU)


def device():
    global _GPU_SEEN
    if not _GPU_SEEN:
        if not torch.cuda.is_available():
            raise _lib.PiccoloHipError("piccolo_amd needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
        _GPU_SEEN = True
    return torch.device("cuda", torch.cuda.current_device())


def _dev(t, dtype=F32):
    """contiguous tensor of `dtype` on the GPU (detached).  A tensor that already is one is returned as it is (the per-image path of
    make_input passes ~20 of them per call: the detach / to / contiguous round trip was a third of its host time)."""
    if torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and not t.requires_grad and t.is_contiguous() and t.device.index == torch.cuda.current_device():
        return t
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    return t.detach().to(device=device(), dtype=dtype).contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _checked(name, *args):
    """call the C entry point `name`, which returns an error code, and raise on failure"""
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _bytes(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device())


def _order_and_buffer(xyz, n, order, sort, nbytes):
    """-> (order, a packed buffer of nbytes) of an n-point cloud.  order maps packed slot -> point index: `order` as computed before for the
    same xyz (checked), else sorted here (pcl_cloud_order), else None (sort False, or a single point: the original order).  The buffer is
    allocated while the sort's workspace is alive: in that block the cloud makes the trim launch 10 % slower."""
    ws = None
    if order is not None:
        if order.dtype != torch.int64 or order.numel() != n or not order.is_cuda:
            raise ValueError("order must be a CUDA int64 tensor with one entry per point")
    elif sort and n > 1:
        order = torch.empty(n, dtype=torch.int64, device=xyz.device)
        nws = _lib.load().pcl_cloud_order_workspace_bytes(n)
        ws = _bytes(nws)
        _checked("pcl_cloud_order", _ptr(xyz), n, _ptr(order), _ptr(ws), nws, _stream())
    return order, _bytes(nbytes)


class Cloud:
    """Point cloud packed for the loss kernel: 6 SoA planes, by default in Morton order of xyz.

    `order` maps packed slot -> original point index (None if the original order was kept).  `color_sets`: how many colourings of the
    points the buffer holds (1 here; Cloud.with_color_sets packs several).  `weights`: None, or the packed plane of per-point weights
    (build-defined, include/piccolo_hip.h): sampling_loss and GradientDescent then evaluate the weighted loss; everything else refuses
    such a cloud (ValueError) — weights are never silently dropped."""

    color_sets = 1
    weights = None

    def __init__(self, xyz, rgb, sort=True, order=None, weights=None):
        """`order`: a Morton order computed before for the same xyz (Cloud(...).order): skips the sort, e.g. when only
        the colours of a cloud changed (color_mod gives every query image its own rgb).  `weights`: (N,) non-negative finite floats in
        the order of xyz's rows."""
        lib = _lib.load()
        xyz, rgb = _dev(xyz), _dev(rgb)
        if xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
            raise ValueError("xyz and rgb must both be (N, 3)")
        self.n = int(xyz.shape[0])
        if self.n <= 0:
            raise ValueError("empty point cloud")
        self.order, self.data = _order_and_buffer(xyz, self.n, order, sort, lib.pcl_cloud_bytes(self.n))
        _checked("pcl_cloud_pack", _ptr(xyz), _ptr(rgb), _ptr(self.order), self.n, _ptr(self.data), _stream())
        self.xyz = xyz          # kept for quantile_box (reads the reference's AoS layout)
        if weights is not None:
            self.set_weights(weights)

    def set_weights(self, w):
        """Pack the (N,) weights `w` (the order of xyz's rows) into this cloud's weight plane — IN PLACE when it has one, so that an engine's
        captured graph reads the new weights.  Negative, NaN or infinite weights raise ValueError (one 4-byte D2H read), and so does None:
        a weighted cloud stays weighted."""
        lib = _lib.load()
        if self.color_sets > 1:
            raise ValueError("set_weights: a cloud of colour sets takes no weights")
        if w is None:
            raise ValueError("set_weights: None (a weighted cloud stays weighted; pack a new Cloud)")
        w = _dev(w)
        if w.dim() != 1 or w.numel() != self.n:
            raise ValueError("weights must be (N,) with one entry per point")
        plane = self.weights if self.weights is not None else torch.empty(lib.pcl_cloud_weights_bytes(self.n) // 4, dtype=F32, device=w.device)
        bad = torch.zeros(1, dtype=torch.int32, device=w.device)
        _checked("pcl_cloud_pack_weights", _ptr(w), _ptr(self.order), self.n, _ptr(plane), _ptr(bad), _stream())
        if int(bad.item()) != 0:
            if self.weights is not None:
                self.weights.zero_()         # (the plane holds the refused values: no vote rather than a wrong one)
            raise ValueError("weights must be non-negative and finite")
        self.weights = plane

    def weighted_view(self, plane):
        """A Cloud that SHARES this one's packed buffer, order and xyz and carries `plane` as its weight plane (the packed plane of
        pcl_cloud_pack_weights / robust_weights: pcl_cloud_stride(n) float32 on the GPU, used as it is — not copied, not checked).  This
        cloud itself stays as it is: a cached unweighted pack never becomes weighted through a view."""
        if self.color_sets > 1:
            raise ValueError("weighted_view: a cloud of colour sets takes no weights")
        if not (torch.is_tensor(plane) and plane.is_cuda and plane.dtype == F32 and plane.is_contiguous()
                and plane.numel() == _lib.load().pcl_cloud_stride(self.n)):
            raise ValueError("weighted_view: the plane must be a contiguous float32 GPU tensor of pcl_cloud_stride(n) entries")
        c = Cloud.__new__(Cloud)
        c.n, c.order, c.xyz, c.data = self.n, self.order, self.xyz, self.data
        c.weights = plane
        return c

    @classmethod
    def private_copy(cls, other):
        """A Cloud with its own packed buffer holding `other`'s contents (same point order): for an engine whose captured graph
        must keep one cloud address while the colours change from image to image."""
        c = cls.__new__(cls)
        c.n, c.order, c.xyz = other.n, other.order, other.xyz
        c.color_sets = other.color_sets
        c.data = other.data.clone()
        c.weights = other.weights.clone() if other.weights is not None else None
        return c

    @classmethod
    def with_color_sets(cls, xyz, rgbs, order=None, sort=True):
        """ONE point set with several colourings (pcl_cloud_pack_sets): planes x, y, z, then (-r, -g, -b) per entry of `rgbs` (a list of
        (N, 3) tensors — e.g. color_mod's per-image colours).  Colour set i is what Cloud(xyz, rgbs[i], order=...) packs, in the same point
        order.  The kernels that take such a cloud (trim_loss_tables, hist_trim_scores_images, GradientDescent) let query image i read
        set i.  Raises ValueError past the 32-bit addressing limit (max_color_sets): split the images into groups."""
        lib = _lib.load()
        xyz = _dev(xyz)
        rgbs = [_dev(r) for r in rgbs]
        if xyz.dim() != 2 or xyz.shape[1] != 3 or not rgbs or any(r.shape != xyz.shape for r in rgbs):
            raise ValueError("xyz and every rgb must be (N, 3)")
        c = cls.__new__(cls)
        c.n = int(xyz.shape[0])
        if c.n <= 0:
            raise ValueError("empty point cloud")
        nbytes = lib.pcl_cloud_sets_bytes(c.n, len(rgbs))
        if nbytes == 0:
            raise ValueError("%d colour sets of %d points exceed the cloud's 32-bit addressing (at most %d)" % (len(rgbs), c.n, max_color_sets(c.n)))
        c.order, c.data = _order_and_buffer(xyz, c.n, order, sort, nbytes)
        c.color_sets = len(rgbs)
        arr = (ctypes.c_void_p * len(rgbs))(*[r.data_ptr() for r in rgbs])
        _checked("pcl_cloud_pack_sets", _ptr(xyz), arr, len(rgbs), _ptr(c.order), c.n, _ptr(c.data), _stream())
        c.xyz = xyz
        return c


def max_color_sets(n):
    """The most colour sets a cloud of n points can hold (pcl_cloud_sets_bytes: 3 + 3 k planes below 2^31 bytes); 0 if n is out of range."""
    lib = _lib.load()
    if lib.pcl_cloud_sets_bytes(n, 1) == 0:
        return 0
    plane = 4 * lib.pcl_cloud_stride(n)
    k = max(1, ((1 << 31) - 1) // plane // 3 - 1)
    while k > 1 and lib.pcl_cloud_sets_bytes(n, k) == 0:
        k -= 1
    return k


class Pano:
    """Query panorama (H,W,3) float packed as zero-bordered texels.

    fmt="auto": fp16-level texels (half4, 8 B) when every value is exactly k/255 in fp32 (what an 8-bit image file
    divided by 255 gives, i.e. everything the reference's harness produces), float4 texels otherwise.  "u8" packs the
    same k/255 images as RGBA8 (4 B/texel: half the footprint, ~5 % slower loss kernel), "f32" forces float4.  The
    exactness test is one kernel and one 4-byte D2H read per image, outside the GD loop."""

    _PACK = {"f16": ("pcl_pano_pack_f16", _lib.PANO_F16), "u8": ("pcl_pano_pack_u8", _lib.PANO_U8),
             "u8p": ("pcl_pano_pack_u8p", _lib.PANO_U8P),         # u8p: rows interleaved in pairs, u8v: vertical pairs — trim launch only
             "u8v": ("pcl_pano_pack_u8v", _lib.PANO_U8V)}
    texels = property(lambda self: (self.H, self.W, self.fmt))      # what the panoramas of one launch share

    def __init__(self, img, fmt="auto"):
        lib = _lib.load()
        src = img
        img = _dev(img)
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("img must be (H, W, 3)")
        self.H, self.W = int(img.shape[0]), int(img.shape[1])
        self.fmt = None
        if fmt not in ("auto", "f16", "u8", "u8p", "u8v", "f32"):
            raise ValueError("unknown texel format %r" % (fmt,))
        prefer = "f16"
        if fmt == "auto":                                     # (experiments: what "auto" tries first)
            prefer = EXPERIMENT.pano_fmt or "f16"
            if prefer == "f32":
                fmt = "f32"
        if fmt != "f32":
            fn, code = self._PACK[prefer if fmt == "auto" else fmt]
            data = _bytes(lib.pcl_pano_bytes(self.H, self.W, code))
            # an image tagged as k/255 by construction (synth.mark_levels: the harness's decoded image files) is not waited for:
            # reading the flag is a blocking D2H copy per query image in front of a millisecond of work — and a flag nobody reads
            # need not be zeroed first (a scratch word per device instead of a fill launch per image)
            known = _known_levels(src)
            flag = _scratch_flag(img.device) if known else torch.zeros(1, dtype=torch.int32, device=img.device)
            _checked(fn, _ptr(img), self.H, self.W, _ptr(data), _ptr(flag), _stream())
            if known or int(flag.item()) == 0:
                self.fmt, self.data = code, data
            elif fmt != "auto":
                raise ValueError("image is not exactly k/255: cannot use %s texels" % fmt)
        if self.fmt is None:
            self.fmt = _lib.PANO_F32
            self.data = _bytes(lib.pcl_pano_bytes(self.H, self.W, _lib.PANO_F32))
            _checked("pcl_pano_pack", _ptr(img), self.H, self.W, _ptr(self.data), _stream())


PYRAMID_MAX_LEVELS = 4      # PCL_PYR_MAX_LEVELS: coarse levels of one pcl_pano_pyramid call
_PYRAMID_FMTS = {"f16": _lib.PANO_F16, "u8": _lib.PANO_U8, "f32": _lib.PANO_F32}


def pyramid_shape(H, W, levels, who="PanoPyramid"):
    """ValueError unless `levels` is an int in 1 .. PYRAMID_MAX_LEVELS and H and W are multiples of 2^levels (pcl_pano_pyramid's refusals,
    on the host: no library, no device) -> levels"""
    if not isinstance(levels, int) or isinstance(levels, bool) or not 1 <= levels <= PYRAMID_MAX_LEVELS:
        raise ValueError("%s: levels %r: an int in 1 .. %d" % (who, levels, PYRAMID_MAX_LEVELS))
    if int(H) <= 0 or int(W) <= 0 or int(H) % (1 << levels) or int(W) % (1 << levels):
        raise ValueError("%s: a %d x %d image has no %d coarse levels (H and W must be multiples of %d)" % (who, H, W, levels, 1 << levels))
    return levels


class _PanoLevel:
    """One coarse level of a PanoPyramid: what the engines read of a Pano (H, W, fmt, data, texels); `data` is a view of the pyramid's
    one buffer, which it keeps alive."""
    texels = property(lambda self: (self.H, self.W, self.fmt))

    def __init__(self, H, W, fmt, data):
        self.H, self.W, self.fmt, self.data = H, W, fmt, data


class PanoPyramid:
    """The query panorama and its coarse levels, packed for the loss kernel (pcl_pano_pyramid, ONE launch for all coarse levels; the rule:
    include/piccolo_hip.h — aligned 2 x 2 blocks of the level below, black pixels are "no data" and leave the mean, a block with data
    never comes out black; a plain box pyramid, no latitude weighting).  The image must be exactly k/255 (ValueError otherwise; an image
    tagged by synth.mark_levels is not waited for, as in Pano).

    .panos[0] is Pano(img) — or `pano0`, the level-0 Pano a caller has packed already —, .panos[l] level l over this object's buffer, in
    the texel format fmts[l - 1] ("f16" | "u8" | "f32"; one string: every level's); default: refine_texels(n, h, w) of the level's size
    when the point count `n` is given, else "f16".  "f16" and "u8" give the same loss bits, so that choice affects speed only.
    images=True: .images holds the float (h, w, 3) level images as well (level 1 first)."""

    def __init__(self, img, levels, fmts=None, n=None, pano0=None, images=False):
        lib = _lib.load()
        src = img
        if not torch.is_tensor(img):
            img = torch.as_tensor(img)
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("img must be (H, W, 3)")
        H, W = int(img.shape[0]), int(img.shape[1])
        self.levels = pyramid_shape(H, W, levels)
        if fmts is None or isinstance(fmts, str):
            fmts = [fmts or (refine_texels(n, H >> l, W >> l) if n is not None else "f16") for l in range(1, levels + 1)]
        fmts = list(fmts)
        if len(fmts) != levels or any(f not in _PYRAMID_FMTS for f in fmts):
            raise ValueError("PanoPyramid: fmts %r: one of %s per coarse level" % (fmts, sorted(_PYRAMID_FMTS)))
        if pano0 is not None and pano0 is not False and (pano0.H, pano0.W) != (H, W):
            raise ValueError("PanoPyramid: pano0 is not this image's size")
        img = _dev(img)
        if img.data_ptr() % 8:                                # (the kernel reads pixel pairs as 8-byte words)
            img = img.clone()
        codes = (ctypes.c_int * levels)(*[_PYRAMID_FMTS[f] for f in fmts])
        nbytes = lib.pcl_pano_pyramid_bytes(H, W, levels, codes)
        if nbytes == 0:
            raise ValueError("PanoPyramid: pcl_pano_pyramid_bytes refuses %d x %d with %d levels" % (H, W, levels))
        # (an OUTPUT, of which the call writes every byte — tests/test_pyramid.py runs it into poisoned buffers —, not a workspace)
        self.buffer = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        sizes = [(H >> l, W >> l) for l in range(1, levels + 1)]
        flat = torch.empty(sum(3 * h * w for h, w in sizes), dtype=F32, device=img.device) if images else None
        known = _known_levels(src)
        flag = _scratch_flag(img.device) if known else torch.zeros(1, dtype=torch.int32, device=img.device)
        _checked("pcl_pano_pyramid", _ptr(img), H, W, levels, codes, _ptr(self.buffer), _ptr(flat), _ptr(flag), _stream())
        if not known and int(flag.item()) != 0:
            raise ValueError("image is not exactly k/255: no pyramid (the rule works on the levels k)")
        # (pano0=False: no level 0 at all — pano_pyramid wants the level images alone)
        self.panos, self.images, off, at = [Pano(src) if pano0 is None else (pano0 or None)], None if flat is None else [], 0, 0
        for (h, w), f in zip(sizes, fmts):
            size = lib.pcl_pano_bytes(h, w, _PYRAMID_FMTS[f])
            self.panos.append(_PanoLevel(h, w, _PYRAMID_FMTS[f], self.buffer[off:off + size]))
            off += (size + 255) // 256 * 256
            if flat is not None:
                self.images.append(flat[at:at + 3 * h * w].view(h, w, 3))
                at += 3 * h * w


def pano_pyramid(img, levels):
    """[level 1, ..., level `levels`] of the (H, W, 3) image of exact levels k/255: float (H >> l, W >> l, 3) GPU tensors, every value
    again exactly k/255 (PanoPyramid's rule and refusals)."""
    return PanoPyramid(img, levels, fmts="u8", pano0=False, images=True).images


_SCRATCH_FLAGS = {}


def _same_texels(panos, p0, complaint="all panoramas of a launch must share size and texel format"):
    """every panorama of a launch has p0's size and texel format"""
    if any(p.texels != p0.texels for p in panos):
        raise ValueError(complaint)


def _scratch_flag(dev):
    """a device int32 the pack kernels may write their `not_exact` answer to when nobody will read it"""
    f = _SCRATCH_FLAGS.get(dev)
    if f is None:
        f = _SCRATCH_FLAGS[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return f


def refine_texels(n, H, W):
    """Level-texel format ("f16" | "u8") for the REFINEMENT of an n-point cloud against an H x W panorama.  fp16-level texels (8 B)
    save 6 VALU instructions per point-pose and win where the loss kernel is VALU-bound (cfg 2: +4-5 % for starting poses near each
    other); a sparse cloud is bound by texture lines, latency and the L2 residency of the texture instead (the 2 x 2 footprints of a
    wave's 128 Morton neighbours share no cache line), and RGBA8 texels (4 B: half the texture in L2) win.  Measured per GD iteration,
    32 candidates all over the room (what make_input hands over; tools/refine_fmt_sweep.sh), f16 -> u8:
        2048 x 1024: 167k points x 6 candidates 14.1 -> 12.0 us; 32 candidates: 400k 66.3 -> 57.2, 700k 86.5 -> 83.1, 1M 112.4 -> 109.6,
                     2M 195.5 -> 199.4 (and with the candidates make_input really trims to at 1M: 11.4 -> 11.55 ms per refinement)
        4096 x 2048: 2M 344.7 -> 226.7, 3M 348.0 -> 318.9, 4M 410.7 -> 407.3, 4.5M 455.1 -> 456.7, 6M 581.6 -> 589.3, 8M 760.1 -> 766.9
    i.e. RGBA8 up to ~0.5 points per pixel for spread poses at both sizes; the threshold sits at 0.45 so that cfg 2 (0.48 points per
    pixel, where poses near each other — bench.py's — run 4-5 % faster on fp16 levels) stays on fp16.  (Round 4's threshold was 1/3:
    it left 8 % on the table at 3M points on 4096 x 2048 — 20 % before the chunks of large clouds were made smaller, pcl_plan.)  The formats give the same bits
    (tests/test_hip_parity.py::test_pano_format_selection_and_float_image)."""
    return "u8" if 20 * int(n) < 9 * int(H) * int(W) else "f16"


def trim_texels(n, H, W):
    """Level-texel layout ("u8p" | "u8" | "u8v") for the TRIM launch of an n-point cloud against an H x W panorama.  Three layouts of the
    same RGBA8 texels, bit-identical tables (tools/trim_u8p.py, tests/test_hip_parity.py::test_trim_loss_table_yaw_shared_vs_generic_
    kernel_and_oracle): plain rows `u8` (two 8-byte accesses per 2 x 2 footprint), rows interleaved in pairs `u8p` (1.5 accesses, same
    bytes, four selects per sample), vertical pairs `u8v` (ONE access, twice the texture).  Which one is fastest depends on what the
    launch is bound by — texture lines (sparse clouds), L2 residency of the texture under hundreds of concurrent views (large
    panoramas), VALU issue (dense clouds) — measured per 1800-pose launch, ms (u8 / u8p / u8v), chunks of at most 16k points
    (pcl_plan_for_groups):
        1024 x  512, u8v = 4 MB : 100k points 0.51 / 0.45 / 0.40, 250k 0.84 / 0.87 / 0.73, 500k 1.47 / 1.62 / 1.35    -> u8v always
        2048 x 1024, u8v = 17 MB: 167k 1.02 / 0.85 / 1.24, 400k 1.72 / 1.51 / 1.94, 700k 2.5 / 2.5 / 2.5, 850k 2.84 / 2.88 / 2.80,
                                  1M 3.18 / 3.34 / 3.06, 2M 6.05 / 6.47 / 5.31, 3M 8.29 / 9.60 / 7.78
                                                                                 -> u8p below 1/3 point per pixel, u8v from 5/12
        4096 x 2048, u8v = 67 MB: 3M 11.1 / 10.2 / 13.6, 4M 13.1 / 13.4 / 14.7, 6M 17.7 / 19.8 / 16.9, 8M 22.8 / 26.1 / 21.2,
                                  10M 28.0 / 32.5 / 26.2                         -> u8p below 0.45 points per pixel, u8v from 0.6
    (With the 64 chunks per launch of rounds 3-4 the large panorama looked different — 10M points 30.4 / 32.0 / 33.4: every chunk was
    a large piece of the room, and the doubled texture lost.)  Sizes in between take the rule of the nearer measured class (by the
    bytes of the doubled texture: up to 6 MB it lives in one XCD's L2, up to 24 MB it is cfg 2's class)."""
    n, px = int(n), int(H) * int(W)
    doubled = 8 * (int(H) + 2) * (int(W) + 2)
    if doubled <= 6_000_000:
        return "u8v"
    if doubled <= 24_000_000:
        return "u8p" if 3 * n < px else "u8v" if 12 * n >= 5 * px else "u8"
    return "u8p" if 20 * n < 9 * px else "u8v" if 5 * n >= 3 * px else "u8"


def trim_order_pays(n, H, W, fmt):
    """Does the trim launch of an n-point cloud against an H x W panorama in texel layout `fmt` (code) take the row-sorted work list
    (TrimOrder)?  Measured per 1800-pose launch, plain (chunk, slot) order -> with the list (tools/trim_u8p.py, round 6; tables bit-identical):
        2048 x 1024: 167k u8p 0.83 -> 0.74 ms, 400k u8p 1.51 -> 1.44, 1M u8v 3.17 -> 3.07 (memory-side 16.4 -> 6.6 GB, L2 hit 0.70 -> 0.88),
                     2M u8v 5.78 -> 5.52; 8 images per launch: 167k 0.747 -> 0.685 per image, 1M 3.10 -> 3.05
        1024 x  512: 100k u8v 0.38 -> 0.38, 500k 1.36 -> 1.35                                      (the texture lives in one L2 either way)
        4096 x 2048: 3M u8p 10.19 -> 10.48 (u8 11.2 -> 11.8, u8v 13.6 -> 13.1), 10M u8v 26.18 -> 26.46 (u8 27.8 -> 28.6)
    i.e. always up to cfg 2's texture class and never above it: for every layout ops.trim_texels picks on a 4096 x 2048 panorama the list
    loses 1-3 % (a band of a 67 MB texture is several L2s wide whatever the order; cfg 5's launch stays at round 5's 26.2 ms)."""
    doubled = 8 * (int(H) + 2) * (int(W) + 2)
    return doubled <= 24_000_000


def _known_levels(img):
    """True for a tensor tagged by synth.mark_levels (every value exactly k/255 by construction); EXPERIMENT.verify_levels ignores
    the tag (the device-side check is then read back as for any other tensor)."""
    tag = getattr(img, "_pcl_levels", None)
    return tag is not None and torch.is_tensor(img) and tag == img._version and not EXPERIMENT.verify_levels


def default_depth(n, H, W, stride=0):
    """(depth_h, depth_w, tau, stride) of pcl_depth_default: the scatter-min depth mask's grid, tolerance and occluder stride for an
    n-point cloud seen in an H x W panorama (>= 12 occluder samples per cell, never finer than the panorama; tau = 3.5 pi / depth_h
    in [0.02, 0.15]; stride 0: the largest of 1, 2, 4 that keeps depth_h >= 128)."""
    dh, dw, tau, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_float(0), ctypes.c_int(0)
    _checked("pcl_depth_default", int(n), int(H), int(W), int(stride), ctypes.byref(dh), ctypes.byref(dw), ctypes.byref(tau), ctypes.byref(st))
    return dh.value, dw.value, tau.value, st.value


def default_depth_res(n, H, W, stride=0):
    return default_depth(n, H, W, stride)[:2]


def depth_tau_rule(depth_h):
    """the tolerance pcl_depth_default attaches to a grid of depth_h rows"""
    return min(max(3.5 * 3.141592653589793 / max(int(depth_h), 1), 0.02), 0.15)


def _depth_args(n, H, W, depth_res, depth_tau, depth_stride=None):
    """(depth_h, depth_w, tau, stride) from the optional cfg values: missing pieces come from pcl_depth_default; a given grid
    without a tolerance gets the rule's tolerance FOR THAT GRID, without a stride every point builds the z-buffer."""
    if depth_res is None:
        dh, dw, tau, st = default_depth(n, H, W, int(depth_stride or 0))
    else:
        dh, dw = int(depth_res[0]), int(depth_res[1])
        tau, st = depth_tau_rule(dh), int(depth_stride or 1)
    if depth_tau is not None:
        tau = float(depth_tau)
    return dh, dw, float(tau), st


def _chain_depth_args(ns, H, W, depth_res, depth_tau, depth_stride=None):
    """(depth_h, depth_w, tau, stride) for the hyper-parameters of ONE depth-masked chain over clouds of `ns` points
    (pcl_gd_run_depth_chain): without depth_res 0 x 0 and the caller's stride (or 0), so that every room resolves its own default grid
    and stride as a run of that room alone does.  The chain has ONE tolerance: rooms whose own tolerances (_depth_args) differ — default
    grids of 80 rows and more without an explicit depth_tau — cannot share it and raise ValueError (omniloc groups its rooms by it)."""
    per = [_depth_args(n, H, W, depth_res, depth_tau, depth_stride) for n in ns]
    if len({p[2] for p in per}) > 1:
        raise ValueError("a depth-masked chain has one tolerance: the rooms' default tolerances differ (%s): pass depth_tau"
                         % sorted({round(p[2], 4) for p in per}))
    if depth_res is None:
        return 0, 0, per[0][2], int(depth_stride or 0)
    return per[0]


def _unweighted(cloud, who):
    """weights are never silently dropped: what takes no weights refuses a weighted cloud"""
    if getattr(cloud, "weights", None) is not None:
        raise ValueError("%s: the cloud carries per-point weights, which only sampling_loss and GradientDescent evaluate" % who)


def sampling_loss(cloud, pano, trans, rot, with_grad=True, visible=None, depth=None):
    """(B, 8) float tensor on the GPU: loss, count, dL/dt(3), dL/d(yaw, pitch, roll).
    A cloud with weights (Cloud(weights=...)): the weighted loss, column 1 the sum of the kept points' weights; not with visible / depth.
    visible: (B, n) uint8 mask in packed point order.  depth: True, or a dict with optional depth_res / depth_tau / depth_stride — the
    scatter-min depth mask of the SAME poses is built and looked up inside the launch (pcl_sampling_loss_depth)."""
    lib = _lib.load()
    trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
    B = int(trans.shape[0])
    if rot.shape[0] != B:
        raise ValueError("trans and rot must have the same number of rows")
    out = torch.empty(B, _lib.RESULT_STRIDE, dtype=F32, device=trans.device)
    if cloud.weights is not None:
        if visible is not None or depth:
            raise ValueError("sampling_loss: per-point weights combine with neither a byte mask (visible) nor depth")
        ws_bytes = lib.pcl_loss_workspace_bytes(cloud.n, B)
        ws = _bytes(ws_bytes)
        _checked("pcl_sampling_loss_weighted", _ptr(cloud.data), _ptr(cloud.weights), cloud.n, _ptr(pano.data), pano.fmt, pano.H, pano.W, _ptr(trans),
                 _ptr(rot), B, 1 if with_grad else 0, _ptr(out), _ptr(ws), ws_bytes, _stream())
        return out
    if depth:
        if visible is not None:
            raise ValueError("sampling_loss: pass either a byte mask (visible) or depth, not both")
        d = depth if isinstance(depth, dict) else {}
        dh, dw, tau, st = _depth_args(cloud.n, pano.H, pano.W, d.get("depth_res"), d.get("depth_tau"), d.get("depth_stride"))
        ws_bytes = lib.pcl_loss_depth_workspace_bytes(cloud.n, B, pano.H, pano.W, dh, dw, st)
        if ws_bytes == 0:
            raise _lib.PiccoloHipError("pcl_loss_depth_workspace_bytes: invalid depth grid %dx%d" % (dh, dw))
        ws = _bytes(ws_bytes)
        _checked("pcl_sampling_loss_depth", _ptr(cloud.data), cloud.n, _ptr(pano.data), pano.fmt, pano.H, pano.W, _ptr(trans), _ptr(rot), B,
                 1 if with_grad else 0, dh, dw, tau, st, _ptr(out), _ptr(ws), ws_bytes, _stream())
        return out
    ws_bytes = lib.pcl_loss_workspace_bytes(cloud.n, B)
    ws = _bytes(ws_bytes)
    vis = None
    if visible is not None:
        vis = _dev(visible, torch.uint8).reshape(B, cloud.n)
    _checked("pcl_sampling_loss", _ptr(cloud.data), cloud.n, _ptr(pano.data), pano.fmt, pano.H, pano.W, _ptr(trans), _ptr(rot), B, 1 if with_grad else 0,
             _ptr(vis), _ptr(out), _ptr(ws), ws_bytes, _stream())
    return out


def _residual_cloud(cloud, pano, who, images=None):
    """images: how many panoramas the call takes, one per colour set (None: one panorama, one colour set only)"""
    if cloud.color_sets > 1 and cloud.color_sets != images:
        raise ValueError("%s: a cloud of colour sets (one colour set only)" % who if images is None else
                         "%s: %d colour sets for %d images" % (who, cloud.color_sets, images))
    if pano.fmt not in (_lib.PANO_F32, _lib.PANO_U8, _lib.PANO_F16):
        raise ValueError("%s: the trim launch's texel layouts (u8p, u8v) are not sampled here" % who)


def _winner_poses(winners, who, rows=None):
    """a (G, 16) tensor as _GdEngine.winners returns it, read on the device -> (trans_ptr, rot_ptr, 16, G): pose stride 16, translation in
    columns 0-2, yaw / pitch / roll in 13-15 — no host round trip between a chain and what is evaluated at its winners.  rows: the row
    count it must have (one per panorama)"""
    ok = torch.is_tensor(winners) and winners.is_cuda and winners.dtype == F32 and winners.is_contiguous() and winners.dim() == 2 \
        and winners.shape[1] == 16 and (winners.shape[0] > 0 if rows is None else winners.shape[0] == rows)
    if not ok:
        raise ValueError("%s: winners must be a contiguous %s float32 GPU tensor" % (who, "(G, 16)" if rows is None else "(I, 16)")
                         + ("" if rows is None else ", one row per panorama"))
    return _ptr(winners), ctypes.c_void_p(winners.data_ptr() + 13 * 4), 16, int(winners.shape[0])


def _depth_form(who, cloud, pano, depth, return_visible=False):
    """The depth= keyword of the single-cloud residual / information / polish functions, sampling_loss's convention (True, or a dict with
    optional depth_res / depth_tau / depth_stride, resolved by _depth_args) -> None without it, else (depth_h, depth_w, tau, stride).
    ValueError: return_visible without depth; with depth a weighted cloud or a cloud of colour sets.  Host only."""
    if not depth:
        if return_visible:
            raise ValueError("%s: return_visible goes with depth" % who)
        return None
    if getattr(cloud, "weights", None) is not None:
        raise ValueError("%s: per-point weights do not combine with depth" % who)
    if cloud.color_sets > 1:
        raise ValueError("%s: a cloud of colour sets does not combine with depth" % who)
    d = depth if isinstance(depth, dict) else {}
    return _depth_args(cloud.n, pano.H, pano.W, d.get("depth_res"), d.get("depth_tau"), d.get("depth_stride"))


def _point_residuals_depth(who, cloud, pano, trans_ptr, rot_ptr, stride, rows, dev, packed, out, dz, return_visible):
    """_point_residuals of ONE Pano under the depth mask of the same poses (pcl_point_residuals_depth) -> rows, or (rows, visible)"""
    lib = _lib.load()
    _residual_cloud(cloud, pano, who)
    dh, dw, tau, st = dz
    if out is None:
        out = torch.empty(rows, cloud.n, dtype=F32, device=dev)
    elif not (out.is_cuda and out.dtype == F32 and out.is_contiguous() and out.numel() == rows * cloud.n):
        raise ValueError("%s: out must be a contiguous (G, N) float32 GPU tensor" % who)
    vis = torch.empty(rows, cloud.n, dtype=torch.uint8, device=dev) if return_visible else None
    nws = lib.pcl_point_residuals_depth_workspace_bytes(rows, dh, dw)
    if nws == 0:
        raise ValueError("%s: %d poses on a %dx%d depth grid are out of range" % (who, rows, dh, dw))
    # (a typed torch.empty like the outputs: the memory-contract harness guards and poisons it alike, tests/test_depth_info.py)
    ws = torch.empty(max(int(nws), 16), dtype=torch.uint8, device=dev)
    order = None if packed else _ptr(cloud.order)
    _checked("pcl_point_residuals_depth", _ptr(cloud.data), cloud.n, _ptr(pano.data), pano.fmt, pano.H, pano.W, trans_ptr, rot_ptr, stride, rows, dh, dw, tau,
             st, order, _ptr(out), _ptr(vis), _ptr(ws), nws, _stream())
    return (out, vis) if return_visible else out


def _point_residuals(who, cloud, panos, trans_ptr, rot_ptr, stride, rows, dev, packed, out=None):
    """What the four residual functions do: `rows` poses (pointers and pose stride) against ONE Pano — pcl_point_residuals, any number of
    poses in one launch — or row i against panos[i] and colour set i of a list of Panos — pcl_point_residuals_images -> (rows, N)"""
    several = not isinstance(panos, Pano)
    if several and len(panos) < 1:
        raise ValueError("%s: no panorama" % who)
    p0 = panos[0] if several else panos
    _residual_cloud(cloud, p0, who, len(panos) if several else None)
    if several:
        _same_texels(panos, p0, "%s: all panoramas must share size and texel format" % who)
        if rows != len(panos):
            raise ValueError("%s: one pose per panorama" % who)
    if out is None:
        out = torch.empty(rows, cloud.n, dtype=F32, device=dev)
    elif not (out.is_cuda and out.dtype == F32 and out.is_contiguous() and out.numel() == rows * cloud.n):
        raise ValueError("%s: out must be a contiguous (%s, N) float32 GPU tensor" % (who, "I" if several else "G"))
    order = None if packed else _ptr(cloud.order)
    if several:
        arr = (ctypes.c_uint64 * rows)(*[p.data.data_ptr() for p in panos])
        _checked("pcl_point_residuals_images", _ptr(cloud.data), cloud.n, int(cloud.color_sets), arr, rows, p0.fmt, p0.H, p0.W, trans_ptr, rot_ptr, stride,
                 order, _ptr(out), _stream())
    else:
        _checked("pcl_point_residuals", _ptr(cloud.data), cloud.n, _ptr(p0.data), p0.fmt, p0.H, p0.W, trans_ptr, rot_ptr, stride, rows, order, _ptr(out),
                 _stream())
    return out


def _pose_rows(trans, rot):
    trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
    if rot.shape[0] != trans.shape[0] or trans.shape[0] == 0:
        raise ValueError("trans and rot must have the same, positive number of rows")
    return trans, rot


def point_residuals(cloud, pano, trans, rot, packed=False, depth=None, return_visible=False):
    """(B, N) float GPU tensor: row b holds, per point, the ||c - rgb|| the loss kernel sums at pose (trans[b], rot[b]) where its mask keeps
    the point and exactly -1 where the sampled colour is exactly black (pcl_point_residuals) — in the order of the cloud's xyz rows, or with
    packed=True in the packed slot order (what robust_weights reads).  A cloud's weights play no part.  ValueError: a cloud of colour sets,
    a panorama in one of the trim launch's texel layouts.
    depth (sampling_loss's convention: True, or a dict with optional depth_res / depth_tau / depth_stride): the scatter-min depth mask of the
    SAME poses is built and looked up inside the launch (pcl_point_residuals_depth) — a visible point keeps its value bit for bit, a hidden
    one reads exactly -1; with return_visible=True -> (rows, visible), visible (B, N) uint8 in the rows' order: the depth decision alone,
    which tells "hidden" from "black".  ValueError: depth with a weighted cloud, return_visible without depth.  depth=None: the call above."""
    dz = _depth_form("point_residuals", cloud, pano, depth, return_visible)
    trans, rot = _pose_rows(trans, rot)
    if dz is not None:
        return _point_residuals_depth("point_residuals", cloud, pano, _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device, packed, None, dz,
                                      return_visible)
    return _point_residuals("point_residuals", cloud, pano, _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device, packed)


def point_residuals_at_winners(cloud, pano, winners, packed=False, out=None, depth=None, return_visible=False):
    """point_residuals at the poses of a (G, 16) tensor as _GdEngine.winners returns it, read on the device (_winner_poses).  out: a (G, N)
    tensor to write into.  depth / return_visible: as for point_residuals."""
    who = "point_residuals_at_winners"
    dz = _depth_form(who, cloud, pano, depth, return_visible)
    if dz is not None:
        return _point_residuals_depth(who, cloud, pano, *_winner_poses(winners, who), winners.device, packed, out, dz, return_visible)
    return _point_residuals("point_residuals_at_winners", cloud, pano, *_winner_poses(winners, "point_residuals_at_winners"), winners.device, packed, out)


# The forms of pose_information / gauss_newton_refine — one cloud and one panorama, one cloud and a panorama per pose, rooms x panoramas, one
# cloud and one panorama under the depth mask — by objective; a form that has no row for an objective does not exist.
# -> (pose information: library call, workspace query; polish: library call, workspace query; the calls' argument convention, _pose_args)
_POSE_FORMS = {
    ("single", "l2"): ("pcl_pose_information", "pcl_pose_information_workspace_bytes", "pcl_gn_refine", "pcl_gn_workspace_bytes", "cov"),
    ("images", "l2"): ("pcl_pose_information_images", "pcl_pose_information_workspace_bytes", "pcl_gn_refine_images", "pcl_gn_workspace_bytes", "cov"),
    ("rooms", "l2"): ("pcl_pose_information_rooms", "pcl_pose_information_rooms_workspace_bytes", "pcl_gn_refine_rooms", "pcl_gn_rooms_workspace_bytes",
                      "cov"),
    ("single", "l1"): ("pcl_pose_information_l1", "pcl_pose_information_workspace_bytes", "pcl_gn_refine_l1", "pcl_gn_workspace_bytes", "delta"),
    ("images", "l1"): ("pcl_pose_information_images_l1", "pcl_pose_information_workspace_bytes", "pcl_gn_refine_images_l1", "pcl_gn_workspace_bytes",
                       "delta"),
    ("depth", "l2"): ("pcl_pose_information_depth", "pcl_pose_information_depth_workspace_bytes", "pcl_gn_refine_depth", "pcl_gn_depth_workspace_bytes",
                      "objective"),
    ("depth", "l1"): ("pcl_pose_information_depth", "pcl_pose_information_depth_workspace_bytes", "pcl_gn_refine_depth", "pcl_gn_depth_workspace_bytes",
                      "objective"),
}


def _pose_form(who, key, delta):
    """The row of _POSE_FORMS for form `key`; delta: what gn_objective returned (None: "l2").  ValueError: the form has no such row."""
    row = _POSE_FORMS.get((key, "l2" if delta is None else "l1"))
    if row is None:
        raise ValueError('%s: objective="l1" has no %s form' % (who, key))
    return row


def _pose_args(convention, head, delta, before_cov, cov, after_cov, ws, nws):
    """The arguments of a library call of a row of _POSE_FORMS: the form's `head`, the call's own pointers around cov, workspace and stream.
    "cov": just that; "delta": no cov, and the float delta before the stream; "objective": (objective, delta) behind the head."""
    args = tuple(head) + ((0 if delta is None else 1, delta or 0.0) if convention == "objective" else ()) + tuple(before_cov)
    args += (() if convention == "delta" else (_ptr(cov),)) + tuple(after_cov) + (_ptr(ws), nws)
    return args + ((delta,) if convention == "delta" else ()) + (_stream(),)


GN_OBJECTIVES = ("l2", "l1")
GN_L1_DELTA = 1.0 / 64         # the default delta of objective="l1": about four grey levels, exact in fp32.  A choice, not a derived value.
GN_L1_DELTA_RANGE = (2.0 ** -20, 4.0)


def gn_objective(who, objective="l2", delta=None):
    """None for objective "l2" (or None), else the float delta of objective "l1" (GN_L1_DELTA when not given).  ValueError: an objective
    that is neither string, a delta without "l1", a delta that is not a finite number inside GN_L1_DELTA_RANGE as a float32.  Host only."""
    import math
    if objective is None:
        objective = "l2"
    if not isinstance(objective, str) or objective not in GN_OBJECTIVES:
        raise ValueError("%s: objective %r: one of %s" % (who, objective, list(GN_OBJECTIVES)))
    if objective == "l2":
        if delta is not None:
            raise ValueError('%s: delta goes with objective="l1"' % who)
        return None
    if delta is None:
        return GN_L1_DELTA
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not math.isfinite(delta):
        raise ValueError("%s: delta %r is not a finite number" % (who, delta))
    d = ctypes.c_float(delta).value
    if not GN_L1_DELTA_RANGE[0] <= d <= GN_L1_DELTA_RANGE[1]:
        raise ValueError("%s: delta %r outside [2^-20, 4] as a float32" % (who, delta))
    return float(delta)


def _single_form(cloud, pano):
    """A form is what _pose_information and _gauss_newton take as the form-specific part of a call: form(who, trans_ptr, rot_ptr, stride, rows)
    runs the form's own argument checks and -> (the form's key in _POSE_FORMS, the workspace queries' arguments, the pose count B, the arguments the
    two library calls of the form begin with, up to the poses, and what the queries found out of range when they answer 0).  This one:
    `rows` poses against one cloud and one panorama (the public functions have run _residual_cloud)."""
    def form(who, trans_ptr, rot_ptr, stride, rows):
        head = (_ptr(cloud.data), _ptr(cloud.weights), cloud.n, _ptr(pano.data), pano.fmt, pano.H, pano.W, trans_ptr, rot_ptr, stride, rows)
        return "single", (cloud.n, rows), rows, head, "%d points x %d poses" % (cloud.n, rows)
    return form


def _depth_single_form(cloud, pano, dz):
    """_single_form under the depth mask (dz of _depth_form): one entry point for both objectives, which travel as (objective, delta) behind
    the grid (_pose_args' "objective" convention)"""
    dh, dw, tau, st = dz

    def form(who, trans_ptr, rot_ptr, stride, rows):
        head = (_ptr(cloud.data), cloud.n, _ptr(pano.data), pano.fmt, pano.H, pano.W, trans_ptr, rot_ptr, stride, rows, dh, dw, tau, st)
        return "depth", (cloud.n, rows, dh, dw), rows, head, "%d points x %d poses on a %dx%d depth grid" % (cloud.n, rows, dh, dw)
    return form


def _pose_information(who, form, trans_ptr, rot_ptr, stride, rows, dev, objective="l2", delta=None):
    """What the six pose_information functions do behind their form's checks -> (H, b, stats, cov); objective "l1": the form's L1 row,
    cov None"""
    lib = _lib.load()
    delta = gn_objective(who, objective, delta)
    key, size_args, B, head, what = form(who, trans_ptr, rot_ptr, stride, rows)
    name, size_name, _, _, convention = _pose_form(who, key, delta)
    nws = getattr(lib, size_name)(*size_args)
    if nws == 0:
        raise ValueError("%s: %s are out of range" % (who, what))
    info = torch.empty(B, 48, dtype=F32, device=dev)
    ws = _bytes(nws)
    cov = torch.empty(B, 6, 6, dtype=F32, device=dev) if delta is None else None
    _checked(name, *_pose_args(convention, head, delta, (_ptr(info),), cov, (), ws, nws))
    return info[:, :36].reshape(B, 6, 6), info[:, 36:42], info[:, 42:47], cov


def pose_information(cloud, pano, trans, rot, objective="l2", delta=None, depth=None):
    """(H (B,6,6), b (B,6), stats (B,5) = M, S1, S2, sigma^2, status, cov (B,6,6)), float32 on the GPU: the Gauss-Newton information matrix
    H = sum w m j j^T of the pose theta = (t, yaw, pitch, roll) at every pose (trans[b], rot[b]), b = sum w m l j, and cov = sigma^2 H^-1
    with sigma^2 = S2 / M (pcl_pose_information; build-defined, include/piccolo_hip.h; metres and radians).  A weighted cloud contributes
    its weights, one factor per term.  status 0: fine; 1: nothing kept or something not finite (cov NaN); 2: H not positive definite
    (cov NaN).  ValueError: a cloud of colour sets, a panorama in one of the trim launch's texel layouts.
    objective="l1" (pcl_pose_information_l1; delta: GN_L1_DELTA unless given, inside [2^-20, 4]): the Huber-L1 form the L1 polish works on —
    the tuple keeps its layout, H = sum w m phi j j^T and b = sum w m phi l j with phi = min(1 / l, 1 / delta), stats = (M, S1, sum w m rho,
    F_rho, status) with M and S1 PLAIN (S1 / M is the weighted sampling loss at the pose), and cov is None.  objective="l2" (or absent):
    the call above, bit for bit.  ValueError: an objective that is neither, delta without "l1" or outside its range.
    depth (sampling_loss's convention): every sum runs over the points the depth mask of the SAME poses keeps as well
    (pcl_pose_information_depth: the z-buffers are built at the poses, the pass looks them up); both objectives.  ValueError: depth with a
    weighted cloud.  depth=None: the calls above."""
    _residual_cloud(cloud, pano, "pose_information")
    dz = _depth_form("pose_information", cloud, pano, depth)
    trans, rot = _pose_rows(trans, rot)
    form = _single_form(cloud, pano) if dz is None else _depth_single_form(cloud, pano, dz)
    return _pose_information("pose_information", form, _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device, objective, delta)


def pose_information_at_winners(cloud, pano, winners, objective="l2", delta=None, depth=None):
    """pose_information at the poses of a (G, 16) tensor as _GdEngine.winners returns it, read on the device (_winner_poses)."""
    _residual_cloud(cloud, pano, "pose_information_at_winners")
    dz = _depth_form("pose_information_at_winners", cloud, pano, depth)
    form = _single_form(cloud, pano) if dz is None else _depth_single_form(cloud, pano, dz)
    return _pose_information("pose_information", form, *_winner_poses(winners, "pose_information_at_winners"), winners.device, objective, delta)


GN_HYPER = dict(lam0=1e-3, lam_up=10.0, lam_down=0.1, lam_min=1e-9, lam_max=1e9, step_cap=0.1, tol=0.0)
GN_MAX_ITERS = 1000


def gn_hyper(who="gauss_newton_refine", **hyper):
    """_lib.GnHyper of the defaults GN_HYPER with the given values in their place.  ValueError: an unknown name, what pcl_gn_refine
    refuses (a value that is not finite, lam0 <= 0, lam_up <= 1, lam_down outside (0, 1], lam_min > lam_max, step_cap <= 0, tol < 0)."""
    import math
    h = dict(GN_HYPER)
    for key, v in hyper.items():
        if key not in h:
            raise ValueError("%s: unknown hyper-parameter %r (one of %s)" % (who, key, sorted(h)))
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError("%s: %s = %r is not a finite number" % (who, key, v))
        h[key] = float(v)
    g = _lib.GnHyper(**h)
    if not (g.lam0 > 0 and g.lam_up > 1 and 0 < g.lam_down <= 1 and g.lam_min <= g.lam_max and g.step_cap > 0 and g.tol >= 0
            and all(math.isfinite(getattr(g, key)) for key in h)):
        raise ValueError("%s: hyper-parameters out of range: %r (lam0 > 0, lam_up > 1, 0 < lam_down <= 1, lam_min <= lam_max, step_cap > 0, "
                         "tol >= 0, all finite in float32)" % (who, h))
    return g


def _gauss_newton(who, form, trans_ptr, rot_ptr, stride, rows, dev, iters, trace, hyper, objective="l2", delta=None):
    """What the six gauss_newton_refine functions do: iters, the hyper-parameters, the form's checks, the sizes, the call -> the result dict;
    objective "l1": the form's L1 twin, cov None (objective and delta are not hyper-parameters: gn_hyper refuses them)"""
    lib = _lib.load()
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= GN_MAX_ITERS:
        raise ValueError("%s: iters %r: an int in 0 .. %d" % (who, iters, GN_MAX_ITERS))
    hp = gn_hyper(who, **hyper)
    delta = gn_objective(who, objective, delta)
    key, size_args, B, head, what = form(who, trans_ptr, rot_ptr, stride, rows)
    _, _, name, size_name, convention = _pose_form(who, key, delta)
    nws, nst = getattr(lib, size_name)(*size_args), lib.pcl_gn_state_bytes(B)
    if nws == 0 or nst == 0:
        raise ValueError("%s: %s are out of range" % (who, what))
    out = torch.empty(B, 16, dtype=F32, device=dev)
    info = torch.empty(B, 48, dtype=F32, device=dev)
    cov = torch.empty(B, 6, 6, dtype=F32, device=dev) if delta is None else None
    tr = torch.empty(iters + 1, B, 16, dtype=F32, device=dev) if trace else None
    ws, st = _bytes(nws), _bytes(nst)
    before_cov = (ctypes.byref(hp), iters, _ptr(st), _ptr(out), _ptr(info))
    _checked(name, *_pose_args(convention, head, delta, before_cov, cov, (_ptr(tr),), ws, nws))
    ret = dict(trans=out[:, 0:3], rot=out[:, 3:6], sigma2_start=out[:, 6], sigma2=out[:, 7], lam=out[:, 8], accepted=out[:, 9], rejected=out[:, 10],
               evaluations=out[:, 11], status=out[:, 12], H=info[:, :36].reshape(B, 6, 6), b=info[:, 36:42], stats=info[:, 42:47], cov=cov)
    if trace:
        ret["trace"] = tr
    return ret


def gauss_newton_refine(cloud, pano, trans, rot, iters=10, trace=False, objective="l2", delta=None, depth=None, **hyper):
    """A Levenberg-Marquardt polish of the poses (trans[b], rot[b]) on the device (pcl_gn_refine; build-defined, include/piccolo_hip.h): it
    minimises the MEAN SQUARED residual sigma^2 = sum w m l^2 / sum w m over theta = (t, yaw, pitch, roll; metres, radians) with the H and b
    of pose_information — NOT the sampling loss sum w m l / sum w m; the two share their per-point terms, mask and weights and are
    different objectives.  -> dict of float32 GPU tensors: trans (B,3), rot (B,3) the best accepted pose; sigma2_start, sigma2 (B,): F at the
    caller's pose and at the returned one; lam the final damping; accepted, rejected, evaluations, status (B,) (0 all iters + 1
    evaluations ran, 1 the first had nothing kept or something not finite — the caller's pose comes back —, 2 the damped matrix was
    not positive definite, 3 converged); H, b, stats, cov: pose_information at the returned pose, bit for bit; with trace=True `trace`
    (iters + 1, B, 16): per evaluation theta_try (6), F, accepted, lambda after the decision, M.  hyper: lam0, lam_up, lam_down, lam_min,
    lam_max, step_cap, tol (GN_HYPER).  A weighted cloud contributes its weights.  ValueError: a cloud of colour sets, a panorama in one of
    the trim launch's texel layouts, iters outside 0 .. 1000, hyper-parameters out of range.
    objective="l1" (pcl_gn_refine_l1; delta: GN_L1_DELTA unless given, inside [2^-20, 4]): the same chain on the Huber-L1 objective
    F_rho = sum w m rho(l) / sum w m, rho = l - delta / 2 (l >= delta), l^2 / (2 delta) (l < delta) — for delta -> 0 the sampling loss
    itself —, re-weighted at every evaluation: H, b are pose_information(objective="l1")'s.  The dict keeps its layout: sigma2_start, sigma2
    and the trace's F column hold F_rho, stats is (M, S1, sum w m rho, F_rho, status) with M and S1 plain, cov is None.  objective="l2" (or
    absent): the chain above, bit for bit.  objective and delta are no hyper-parameters (gn_hyper refuses them).
    depth (sampling_loss's convention; pcl_gn_refine_depth): the same chain under the depth mask, REBUILT at every trial pose — the z-buffers
    of all poses are built at the trial poses in front of every evaluation, so a point that the step uncovers counts at once; H, b, stats
    and cov are pose_information(depth=...) at the returned pose, bit for bit.  Both objectives.  ValueError: depth with a weighted cloud.
    depth=None: the chains above.  Nothing is claimed about real data."""
    _residual_cloud(cloud, pano, "gauss_newton_refine")
    dz = _depth_form("gauss_newton_refine", cloud, pano, depth)
    trans, rot = _pose_rows(trans, rot)
    form = _single_form(cloud, pano) if dz is None else _depth_single_form(cloud, pano, dz)
    return _gauss_newton("gauss_newton_refine", form, _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device, iters, trace, hyper, objective,
                         delta)


def gauss_newton_refine_at_winners(cloud, pano, winners, iters=10, trace=False, objective="l2", delta=None, depth=None, **hyper):
    """gauss_newton_refine from the poses of a (G, 16) tensor as _GdEngine.winners returns it, read on the device (_winner_poses)."""
    _residual_cloud(cloud, pano, "gauss_newton_refine_at_winners")
    who = "gauss_newton_refine_at_winners"
    dz = _depth_form(who, cloud, pano, depth)
    form = _single_form(cloud, pano) if dz is None else _depth_single_form(cloud, pano, dz)
    return _gauss_newton(who, form, *_winner_poses(winners, who), winners.device, iters, trace, hyper, objective, delta)


def _images_call(who, cloud, panos, rows, planes):
    """What the images forms of pose_information / gauss_newton_refine check and pass on: one pose per panorama, panoramas of one size and
    texel format, a cloud of one colour set or of one per image (_residual_cloud), and the weights — planes None: the cloud's own plane for
    every image, where it has one; else an (I, pcl_cloud_stride(n)) float32 GPU tensor, plane i for image i (what
    GradientDescent.weight_planes() of a weight-set chain returns).  -> (panos, the host array of their addresses, weights, weight_sets)"""
    panos = list(panos)
    if len(panos) < 1:
        raise ValueError("%s: no panorama" % who)
    I = len(panos)
    _residual_cloud(cloud, panos[0], who, I)
    _same_texels(panos, panos[0], "%s: all panoramas must share size and texel format" % who)
    if rows != I:
        raise ValueError("%s: one pose per panorama" % who)
    if planes is None:
        weights, sets = cloud.weights, 0 if cloud.weights is None else 1
    else:
        if not (torch.is_tensor(planes) and planes.is_cuda and planes.dtype == F32 and planes.is_contiguous()
                and tuple(planes.shape) == (I, _lib.load().pcl_cloud_stride(cloud.n))):
            raise ValueError("%s: planes must be a contiguous (I, pcl_cloud_stride(n)) float32 GPU tensor, one plane per panorama" % who)
        weights, sets = planes, I
    return panos, (ctypes.c_uint64 * I)(*[p.data.data_ptr() for p in panos]), weights, sets


def _images_form(cloud, panos, planes):
    """The form (_single_form) of row i against panos[i]: _images_call's checks"""
    def form(who, trans_ptr, rot_ptr, stride, rows):
        ps, arr, weights, sets = _images_call(who, cloud, panos, rows, planes)
        p0, I = ps[0], len(ps)
        head = (_ptr(cloud.data), _ptr(weights), sets, cloud.n, int(cloud.color_sets), arr, I, p0.fmt, p0.H, p0.W, trans_ptr, rot_ptr, stride)
        return "images", (cloud.n, I), I, head, "%d points x %d poses" % (cloud.n, I)
    return form


def pose_information_images(cloud, panos, trans, rot, planes=None, objective="l2", delta=None):
    """pose_information for I poses, each against ITS OWN panorama, in one set of launches (pcl_pose_information_images): row i of
    (H, b, stats, cov) is pose (trans[i], rot[i]) against panos[i] — and, for a cloud of I colour sets (Cloud.with_color_sets), colour
    set i — under the cloud's own weight plane where it has one (planes=None) or under planes[i] of an (I, pcl_cloud_stride(n)) float32 GPU
    tensor (GradientDescent.weight_planes() of a weight-set chain).  Row i equals pose_information of that pose, panorama, colour set and
    plane alone, bit for bit.  ValueError: as pose_information; a colour-set count that is not the image count; panoramas of different
    sizes or texel formats; planes of another shape.  objective / delta: as pose_information ("l1": pcl_pose_information_images_l1, cov
    None, stats = (M, S1, sum w m rho, F_rho, status)); row i still equals the single call's with the same objective, bit for bit."""
    trans, rot = _pose_rows(trans, rot)
    return _pose_information("pose_information_images", _images_form(cloud, panos, planes), _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device,
                             objective, delta)


def pose_information_images_at_winners(cloud, panos, winners, planes=None, objective="l2", delta=None):
    """pose_information_images at the poses of an (I, 16) tensor as _GdEngine.winners(I) returns it, read on the device (_winner_poses): row
    i is winner i against panos[i] (colour set i, plane i)."""
    who = "pose_information_images_at_winners"
    return _pose_information(who, _images_form(cloud, panos, planes), *_winner_poses(winners, who), winners.device, objective, delta)


def gauss_newton_refine_images(cloud, panos, trans, rot, iters=10, trace=False, planes=None, objective="l2", delta=None, **hyper):
    """gauss_newton_refine for I poses, each against ITS OWN panorama, in ONE chain (pcl_gn_refine_images): pose i = (trans[i], rot[i]) is
    polished against panos[i] — colour set i of a cloud of I colour sets, the cloud's own weight plane (planes=None) or planes[i] as for
    pose_information_images.  -> gauss_newton_refine's dict with one row per image (trace: (iters + 1, I, 16)); row i equals the single
    call's for that pose, panorama, colour set and plane, bit for bit — a pose that freezes moves no other pose's bits.  objective / delta:
    as gauss_newton_refine ("l1": pcl_gn_refine_images_l1; sigma2_start, sigma2 and the trace's F hold F_rho, stats = (M, S1, sum w m rho,
    F_rho, status), cov None)."""
    trans, rot = _pose_rows(trans, rot)
    return _gauss_newton("gauss_newton_refine_images", _images_form(cloud, panos, planes), _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device,
                         iters, trace, hyper, objective, delta)


def gauss_newton_refine_images_at_winners(cloud, panos, winners, iters=10, trace=False, planes=None, objective="l2", delta=None, **hyper):
    """gauss_newton_refine_images from the poses of an (I, 16) tensor as _GdEngine.winners(I) returns it, read on the device (_winner_poses)."""
    who = "gauss_newton_refine_images_at_winners"
    return _gauss_newton(who, _images_form(cloud, panos, planes), *_winner_poses(winners, who), winners.device, iters, trace, hyper, objective, delta)


def _rooms_call(who, clouds, panos, rows):
    """What the rooms forms of pose_information / gauss_newton_refine check and pass on: 1..PCL_GD_MAX_ROOMS unweighted room clouds that all
    hold one colour set or all one per image, panoramas of one size and texel format, one pose per (room, image), room by room.
    -> (clouds, panos, the GdRoom array (no boxes), the host array of the panorama addresses, color_sets)"""
    clouds, panos = list(clouds), list(panos)
    if not 1 <= len(clouds) <= _lib.GD_MAX_ROOMS:
        raise ValueError("%s: %d rooms (1..%d per call)" % (who, len(clouds), _lib.GD_MAX_ROOMS))
    if len(panos) < 1:
        raise ValueError("%s: no panorama" % who)
    I = len(panos)
    for c in clouds:
        if c.weights is not None:
            raise ValueError("%s: a weighted room cloud (the rooms chains take no weights)" % who)
        _residual_cloud(c, panos[0], who, I)
    if len({int(c.color_sets) for c in clouds}) != 1:
        raise ValueError("%s: every room cloud needs one colour set, or one per image (%d)" % (who, I))
    _same_texels(panos, panos[0], "%s: all panoramas must share size and texel format" % who)
    if rows != len(clouds) * I:
        raise ValueError("%s: one pose per (room, panorama): %d poses for %d rooms x %d panoramas" % (who, rows, len(clouds), I))
    rooms = (_lib.GdRoom * len(clouds))(*[_lib.GdRoom(c.data.data_ptr(), c.n, None) for c in clouds])
    return clouds, panos, rooms, (ctypes.c_uint64 * I)(*[p.data.data_ptr() for p in panos]), int(clouds[0].color_sets)


def _rooms_form(clouds, panos):
    """The form (_single_form) of row r * I + i against clouds[r] and panos[i]: _rooms_call's checks"""
    def form(who, trans_ptr, rot_ptr, stride, rows):
        cs, ps, rooms, arr, sets = _rooms_call(who, clouds, panos, rows)
        p0, R, I = ps[0], len(cs), len(ps)
        head = (rooms, R, sets, arr, I, p0.fmt, p0.H, p0.W, trans_ptr, rot_ptr, stride)
        return "rooms", (rooms, R, I), R * I, head, "%d rooms x %d poses" % (R, I)
    return form


def pose_information_rooms(clouds, panos, trans, rot):
    """pose_information for R x I poses in one set of launches (pcl_pose_information_rooms): row r * I + i of (H, b, stats, cov) is pose
    (trans[r * I + i], rot[r * I + i]) against room cloud clouds[r] and panos[i] — and, where every room cloud holds I colour sets
    (Cloud.with_color_sets), colour set i of room r.  That row equals pose_information of that pose, room, colour set and panorama alone,
    bit for bit.  ValueError: as pose_information; more than PCL_GD_MAX_ROOMS rooms; a weighted room cloud; room clouds whose colour-set
    counts differ or are neither 1 nor I; panoramas of different sizes or texel formats; a pose count that is not R * I."""
    trans, rot = _pose_rows(trans, rot)
    return _pose_information("pose_information_rooms", _rooms_form(clouds, panos), _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device)


def pose_information_rooms_at_winners(clouds, panos, winners):
    """pose_information_rooms at the poses of an (R * I, 16) tensor as GradientDescentRoomsImages.winner() returns it, read on the device
    (_winner_poses): row r * I + i is the winner of (room r, image i)."""
    who = "pose_information_rooms_at_winners"
    return _pose_information(who, _rooms_form(clouds, panos), *_winner_poses(winners, who), winners.device)


def gauss_newton_refine_rooms(clouds, panos, trans, rot, iters=10, trace=False, **hyper):
    """gauss_newton_refine for R x I poses in ONE chain (pcl_gn_refine_rooms): pose r * I + i is polished against room cloud clouds[r] and
    panos[i] — colour set i of room r where the room clouds hold I sets.  -> gauss_newton_refine's dict with one row per (room, image),
    room by room (trace: (iters + 1, R * I, 16)); every row equals the single call's for that pose, room, colour set and panorama, bit for
    bit — a pose that freezes moves no other pose's bits.  ValueError: as pose_information_rooms and gauss_newton_refine."""
    trans, rot = _pose_rows(trans, rot)
    return _gauss_newton("gauss_newton_refine_rooms", _rooms_form(clouds, panos), _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device, iters,
                         trace, hyper)


def gauss_newton_refine_rooms_at_winners(clouds, panos, winners, iters=10, trace=False, **hyper):
    """gauss_newton_refine_rooms from the poses of an (R * I, 16) tensor as GradientDescentRoomsImages.winner() returns it, read on the device
    (_winner_poses)."""
    who = "gauss_newton_refine_rooms_at_winners"
    return _gauss_newton(who, _rooms_form(clouds, panos), *_winner_poses(winners, who), winners.device, iters, trace, hyper)


def point_residuals_images(cloud, panos, trans, rot, packed=False):
    """(I, N) float GPU tensor: row i is point_residuals of pose (trans[i], rot[i]) against panos[i] — and, for a cloud of I colour sets
    (Cloud.with_color_sets), colour set i — in ONE launch (pcl_point_residuals_images; the panorama addresses are kernel arguments).  Row i
    equals the single call's row bit for bit.  packed: as point_residuals."""
    trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
    if rot.shape[0] != trans.shape[0]:
        raise ValueError("point_residuals_images: one pose per panorama")
    return _point_residuals("point_residuals_images", cloud, list(panos), _ptr(trans), _ptr(rot), 3, int(trans.shape[0]), trans.device, packed)


def point_residuals_images_at_winners(cloud, panos, winners, packed=False, out=None):
    """point_residuals_images at the poses of an (I, 16) tensor as _GdEngine.winners(I) returns it, read on the device (pose stride 16): row i
    is winner i against panos[i] (and colour set i).  out: an (I, N) tensor to write into."""
    who = "point_residuals_images_at_winners"
    return _point_residuals(who, cloud, list(panos), *_winner_poses(winners, who, len(panos)), winners.device, packed, out)


ROBUST_KINDS = {"trunc": _lib.ROBUST_TRUNC, "huber": _lib.ROBUST_HUBER}


def robust_weights(cloud, residual_row_packed, kind="trunc", k=2.5, plane=None, scale=None):
    """(plane, scale) from ONE row of point_residuals(..., packed=True): scale = (s, M) on the GPU, s the lower median of the row's M
    entries that are not -1, and plane the packed weight plane (pcl_cloud_stride(n) floats, what Cloud.weighted_view takes) of
    kind "trunc": l <= k s ? 1 : 0 or "huber": l <= k s ? 1 : k s / l; a masked point (-1) weighs 1, a NaN or infinite residual 0, and with
    M = 0 every point weighs 1 (pcl_robust_weights).  plane / scale: tensors to write into (a plane a captured graph reads, in place)."""
    return robust_plane(cloud.n, residual_row_packed, kind, k, plane, scale)


def robust_plane(n, row, kind="trunc", k=2.5, plane=None, scale=None):
    """robust_weights for a row of n residuals in any one point order: the plane's first n entries are in that order.  robust_planes on a
    one-row view"""
    row = _dev(row)
    if row.dim() != 1 or row.numel() != n or n <= 0:
        raise ValueError("robust_weights: one residual per point, (N,)")
    if plane is not None and not (plane.is_cuda and plane.dtype == F32 and plane.is_contiguous() and plane.numel() == _lib.load().pcl_cloud_stride(n)):
        raise ValueError("robust_weights: plane must be a contiguous float32 GPU tensor of pcl_cloud_stride(n) entries")
    planes, scales = robust_planes(n, row.view(1, n), kind, k, None if plane is None else plane.view(1, -1), None if scale is None else scale.view(1, 2))
    return planes[0] if plane is None else plane, scales[0] if scale is None else scale


def robust_planes(n, rows, kind="trunc", k=2.5, planes=None, scales=None, ws=None):
    """The robust weights of the R rows of an (R, n) tensor in six launches (pcl_robust_weights_rows): -> (planes (R, pcl_cloud_stride(n)),
    scales (R, 2)); plane i and scale i equal robust_plane(n, rows[i], kind, k) bit for bit.  planes / scales / ws: tensors to write into
    (ws: a byte workspace of pcl_robust_weights_rows_workspace_bytes(n, R))."""
    lib = _lib.load()
    if kind not in ROBUST_KINDS:
        raise ValueError("robust_weights: kind %r (one of %s)" % (kind, sorted(ROBUST_KINDS)))
    k = float(k)
    if not (k > 0.0 and k < float("inf")):
        raise ValueError("robust_weights: k must be positive and finite, got %r" % (k,))
    rows = _dev(rows)
    if rows.dim() != 2 or rows.shape[1] != n or n <= 0 or rows.shape[0] < 1:
        raise ValueError("robust_weights: rows of one residual per point, (R, N)")
    R, stride = int(rows.shape[0]), lib.pcl_cloud_stride(n)
    if planes is None:
        planes = torch.empty(R, stride, dtype=F32, device=rows.device)
    elif not (planes.is_cuda and planes.dtype == F32 and planes.is_contiguous() and planes.numel() == R * stride):
        raise ValueError("robust_weights: planes must be a contiguous float32 GPU tensor of R x pcl_cloud_stride(n) entries")
    if scales is None:
        scales = torch.empty(R, 2, dtype=F32, device=rows.device)
    elif not (scales.is_cuda and scales.dtype == F32 and scales.is_contiguous() and scales.numel() == 2 * R):
        raise ValueError("robust_weights: scales must be a contiguous float32 GPU tensor of R x 2 entries")
    nws = lib.pcl_robust_weights_rows_workspace_bytes(n, R)
    if nws == 0:
        raise ValueError("robust_weights: %d rows of %d points" % (R, n))
    if ws is None:
        ws = _bytes(nws)
    _checked("pcl_robust_weights_rows", _ptr(rows), n, R, ROBUST_KINDS[kind], k, _ptr(planes), _ptr(scales), _ptr(ws), ws.numel(), _stream())
    return planes, scales


TRIM_MAX_ROT = 1024        # pcl_trim_groups: rotations per table (include/piccolo_hip.h)


class TrimGroups:
    """Classes of equal (pitch, roll) of an (R, 3) rotation table, built on the device (pcl_trim_groups) — what trim_loss_table
    needs from the rotation grid.  Built once per grid: the group count is read back here (one 4-byte D2H copy), so that the
    per-image launches are sized exactly."""

    def __init__(self, rot):
        lib = _lib.load()
        self.rot = _dev(rot).reshape(-1, 3)
        self.R = int(self.rot.shape[0])
        if self.R <= 0:
            raise ValueError("empty rotation table")
        self.data = _bytes(lib.pcl_trim_groups_bytes(self.R))
        _checked("pcl_trim_groups", _ptr(self.rot), self.R, _ptr(self.data), _stream())
        self.ngroups = int(self.data[:4].view(torch.int32).item())


class TrimOrder:
    """The trim launch's row-sorted work list (pcl_trim_order): which (cloud chunk, slot) item each block evaluates, ranked by the
    panorama row the chunk lands in so that an XCD's L2 holds a band of the texture for all the poses.  Depends on the cloud, the
    candidate grid and the panorama's size / texel layout — not on the query image: build once per room, pass to trim_loss_table[s]
    (scheduling only: tables are bit-identical with or without it)."""

    def __init__(self, cloud, pano_shape, trans, groups):
        """pano_shape = (H, W, texel format code) of the panoramas the launches will read"""
        lib = _lib.load()
        trans = _dev(trans).reshape(-1, 3)
        H, W, fmt = pano_shape
        self.key = (cloud.n, int(trans.shape[0]), groups.ngroups, int(H), int(W), int(fmt))
        self.data = _bytes(lib.pcl_trim_order_bytes(cloud.n, self.key[1], groups.ngroups))
        nws = lib.pcl_trim_order_workspace_bytes(cloud.n, self.key[1], groups.ngroups)
        ws = _bytes(nws)
        _checked("pcl_trim_order", _ptr(cloud.data), cloud.n, int(fmt), int(H), int(W), _ptr(trans), self.key[1], _ptr(groups.rot), groups.R, _ptr(groups.data),
                 groups.ngroups, _ptr(self.data), _ptr(ws), nws, _stream())


TRIM_MAX_IMAGES = 32       # pcl_trim_loss_images_sets: query images per launch


def _trim_tables(cloud, panos, trans, groups, return_count, order, sets=False):
    """(I, K, R) loss tables (and counts) of the panoramas, TRIM_MAX_IMAGES per launch; sets: image i reads colour set i (one launch)"""
    lib = _lib.load()
    trans = _dev(trans).reshape(-1, 3)
    K, I, p0 = int(trans.shape[0]), len(panos), panos[0]
    table = torch.empty(I, K, groups.R, dtype=F32, device=trans.device)
    count = torch.empty(I, K, groups.R, dtype=F32, device=trans.device) if return_count else None
    for i0 in range(0, I, TRIM_MAX_IMAGES):
        part = panos[i0:i0 + TRIM_MAX_IMAGES]
        nws = lib.pcl_trim_loss_images_workspace_bytes(cloud.n, K, groups.ngroups, len(part))
        ws = _bytes(nws)
        arr = (ctypes.c_void_p * len(part))(*[p.data.data_ptr() for p in part])
        _checked("pcl_trim_loss_images_sets", _ptr(cloud.data), cloud.n, len(part) if sets else 1, arr, len(part), p0.fmt, p0.H, p0.W, _ptr(trans), K,
                 _ptr(groups.rot), groups.R, _ptr(groups.data), groups.ngroups, _ptr(order.data) if order is not None else None, _ptr(table[i0:]),
                 _ptr(count[i0:]) if return_count else None, _ptr(ws), nws, _stream())
    return table, count


def trim_loss_table(cloud, pano, trans, groups, return_count=False, order=None):
    """utils.py:484-499 for all pairs: (K, R) float GPU tensor loss_table[i, j] = forward-only sampling loss of (trans[i], rot[j]),
    rotations of one (pitch, roll) class sharing the projection (csrc/pcl_trim.hip).  order: a TrimOrder of this cloud / grid."""
    _unweighted(cloud, "trim_loss_table")
    table, count = _trim_tables(cloud, [pano], trans, groups, return_count, order)
    return (table[0], count[0]) if return_count else table[0]


def trim_loss_tables(cloud, panos, trans, groups, return_count=False, order=None):
    """trim_loss_table for several query images of one room in ONE launch: (I, K, R) float GPU tensor; image i's table has the
    bits of trim_loss_table(cloud, panos[i], ...) (same chunks of the cloud).  panos: list of Pano of one size / texel format.
    A cloud with colour sets (Cloud.with_color_sets, one per image): image i reads set i — its table is trim_loss_table over
    Cloud(xyz, rgbs[i]), bit for bit."""
    _unweighted(cloud, "trim_loss_tables")
    I, p0 = len(panos), panos[0]
    _same_texels(panos, p0)
    if cloud.color_sets > 1:
        if cloud.color_sets != I:
            raise ValueError("a cloud of %d colour sets for %d images" % (cloud.color_sets, I))
        if I > TRIM_MAX_IMAGES:
            raise ValueError("trim_loss_tables: at most %d images per call with colour sets" % TRIM_MAX_IMAGES)
    table, count = _trim_tables(cloud, panos, trans, groups, return_count, order, sets=cloud.color_sets > 1)
    return (table, count) if return_count else table


def select_poses(values, n_keep, trans, rot, largest=False, rot_per_trans=0, return_idx=False):
    """The selections of the initialisation stage (utils.py:500-505 / :583-586) in one launch: values (M,) or (P, M) -> the
    n_keep best rows (trans[idx // rot_per_trans], rot[idx % rot_per_trans]) — or (trans[idx], rot[idx]) when rot_per_trans is 0
    — in rank order, as ((P,) n_keep, 3) tensors.  Stable order; NaN ranks last.  With (P, M) values, trans / rot are either shared
    2-D tables or (P, rows, 3) stacks."""
    values = _dev(values)
    single = values.dim() == 1
    v = values.reshape(1, -1) if single else values.reshape(values.shape[0], -1)
    P, M = int(v.shape[0]), int(v.shape[1])
    trans, rot = _dev(trans), _dev(rot)
    stride = 0
    if trans.dim() == 3:
        if rot.dim() != 3 or trans.shape[0] != P or rot.shape[:2] != trans.shape[:2]:
            raise ValueError("select_poses: per-problem pose tables must be (P, rows, 3) for both trans and rot")
        stride = int(trans.shape[1])
    trans, rot = trans.reshape(-1, 3), rot.reshape(-1, 3)
    rows_t = trans.shape[0] if stride == 0 else stride
    rows_r = rot.shape[0] if stride == 0 else stride
    need_t = (M + rot_per_trans - 1) // rot_per_trans if rot_per_trans > 0 else M
    need_r = rot_per_trans if rot_per_trans > 0 else M
    if rows_t < need_t or rows_r < need_r:
        raise ValueError("select_poses: %d values need %d translations and %d rotations" % (M, need_t, need_r))
    n_keep = int(n_keep)
    ot = torch.empty(P, n_keep, 3, dtype=F32, device=v.device)
    orr = torch.empty(P, n_keep, 3, dtype=F32, device=v.device)
    oi = torch.empty(P, n_keep, dtype=torch.int32, device=v.device) if return_idx else None
    _checked("pcl_select_poses", _ptr(v), P, M, n_keep, 1 if largest else 0, _ptr(trans), _ptr(rot), int(rot_per_trans), stride, _ptr(ot), _ptr(orr), _ptr(oi),
             _stream())
    if single:
        ot, orr, oi = ot[0], orr[0], (oi[0] if oi is not None else None)
    return (ot, orr, oi) if return_idx else (ot, orr)


SELECT_MAX_KEEP = 1024      # pcl_select_poses: winners per problem (include/piccolo_hip.h)


HIST_MAX_IMAGES = 32       # pcl_hist_trim_scores_images_sets: query images per call
# bytes of point lists one histogram-trim call may hold
HIST_BATCH_BYTES = 8e9


def _hist_workspace(size_of, count, most, halve, last):
    """The histogram stage's one allocation ladder: a workspace of size_of(min(count, most)) bytes; while the allocation fails `count` is
    halved (where the caller can split its work), and the last resort is a workspace of last() bytes — the z-buffer splat's small one.
    -> (workspace, its bytes, count); workspace None where there is no `last` (the caller has another path)."""
    while True:
        nws = size_of(min(count, most))
        try:
            return _bytes(nws), nws, count
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            if halve and count > 1:
                count = (count + 1) // 2
                continue
            nws = last() if last else 0
            return (_bytes(nws) if last else None), nws, count


def hist_workspace_bytes(n, images, cand_per_image, H, W, num_split_h, num_split_w, color_sets=False):
    """bytes of the histogram stage's workspace for `images` query images of cand_per_image candidates each (0: a shape the stage
    refuses).  n = the cloud's points: the tile-binned render's workspace (the z-buffer's size where that render does not apply);
    n = 0: the z-buffer splat's smaller one, which selects that path.  color_sets: a colour set per image."""
    return _lib.load().pcl_hist_trim_images_sets_workspace_bytes(int(n), images if color_sets else 1, images, int(cand_per_image), int(H), int(W),
                                                                 num_split_h, num_split_w)


def _hist_scores(who, imgs, cloud, trans, rot, num_split_h, num_split_w, splat, batch=None):
    """The one driver of the histogram stage (pcl_hist_trim_scores_images_sets, pcl_hist_trim_reduce_images): imgs = I images, trans / rot
    (I, K, 3) -> (scores (I, K), inter, nproj, nimg).  batch (one image): its candidates `batch` at a time over one workspace, then one
    reduce over all K (the carry-over chain runs through the batches).  Otherwise images in groups, each with its reduce — or, with a
    colour set per image, all images in one call."""
    I, K = int(trans.shape[0]), int(trans.shape[1])
    H, W = int(imgs[0].shape[0]), int(imgs[0].shape[1])
    sets = cloud.color_sets > 1
    nblk = (num_split_h - 2) * num_split_w
    dev = imgs[0].device
    inter = torch.empty(I * K, nblk, dtype=F32, device=dev)
    nproj = torch.empty(I * K, nblk, dtype=torch.int32, device=dev)
    nimg = torch.empty(I, nblk, dtype=torch.int32, device=dev)
    scores = torch.empty(I, K, dtype=F32, device=dev)
    t2, r2 = trans.reshape(I * K, 3).contiguous(), rot.reshape(I * K, 3).contiguous()
    n_ws = 0 if splat else cloud.n               # n = 0: the z-buffer splat path's workspace, which selects it

    def size_of(n, m, cpi):
        return hist_workspace_bytes(n, m, cpi, H, W, num_split_h, num_split_w, sets)

    def run(i0, m, k0, cpi, ws, nws):            # images [i0, i0 + m), candidates [k0, k0 + cpi) of each (k0 > 0: one image in batches)
        arr = (ctypes.c_void_p * m)(*[im.data_ptr() for im in imgs[i0:i0 + m]])
        c0 = i0 * K + k0
        _checked("pcl_hist_trim_scores_images_sets", _ptr(cloud.data), cloud.n, m if sets else 1, arr, m, cpi, H, W, _ptr(t2[c0:]), _ptr(r2[c0:]), num_split_h,
                 num_split_w, _ptr(inter[c0:]), _ptr(nproj[c0:]), _ptr(nimg[i0:]), _ptr(ws), nws, _stream())

    def reduce(i0, m):                           # a block with no pixels ends its block row (the reference `break`s there, utils.py:568-571)
        _checked("pcl_hist_trim_reduce_images", _ptr(inter[i0 * K:]), _ptr(nproj[i0 * K:]), _ptr(nimg[i0:]), m, K, num_split_h, num_split_w, _ptr(scores[i0:]),
                 _stream())

    if batch:
        # one batch for the 64 survivors of the loss trim at 1M points (four batches of 16: 2.0 instead of 1.7 ms; 0.8 instead of
        # 0.5 ms at 167k points); a batch is kept within ~8 GB (10M points: 16 candidates at a time).
        batch = max(1, min(batch, K, int(HIST_BATCH_BYTES // max(size_of(n_ws, 1, 1), 1))))
    unit = size_of(n_ws, I if sets else 1, batch or K)                # one batch / one image / all the images
    if unit == 0:
        raise ValueError("%s: need num_split_h >= 3 and blocks of at least one pixel" % who)
    if batch:
        ws, nws, batch = _hist_workspace(lambda b: size_of(n_ws, 1, b), batch, K, True, lambda: size_of(0, 1, 1))
        for k0 in range(0, K, batch):
            run(0, 1, k0, min(batch, K - k0), ws, nws)
        reduce(0, 1)
    elif sets:
        ws, nws, _ = _hist_workspace(lambda m: size_of(n_ws, m, K), I, I, False, lambda: size_of(0, I, K))
        run(0, I, 0, K, ws, nws)
        reduce(0, I)
    else:
        group, i0 = max(1, min(HIST_MAX_IMAGES, I, int(HIST_BATCH_BYTES // unit))), 0
        while i0 < I:
            # like one image's batches: fewer images at a time, and in the end the per-image path with its own fallbacks
            ws, nws, group = _hist_workspace(lambda m: size_of(n_ws, m, K), group, I - i0, True, None)
            m = min(group, I - i0)
            if ws is None:
                scores[i0] = hist_trim_scores(imgs[i0], cloud, trans[i0], rot[i0], num_split_h, num_split_w, splat=splat)
                m = 1
            else:
                run(i0, m, 0, K, ws, nws)
                reduce(i0, m)
            i0 += m
    return scores, inter, nproj, nimg


def hist_trim_scores(img, cloud, trans, rot, num_split_h, num_split_w, batch=64, return_parts=False, splat=False):
    """Histogram-intersection score of every candidate pose (utils.py:510-588): (K,) GPU tensor, higher is better.
    `cloud` is a packed Cloud.  Candidates are processed `batch` at a time.  Workspace per candidate: the point lists of the
    tile-binned render (48 bytes per point in the worst case, plus the tiles' run tables — 2 bytes per point for a 2048 x 1024 panorama: 3.2 GB for 64
    candidates at 1M points; HBM is there to be used),
    or, where that path does not apply (more than 4096 image tiles, ...) or does not fit, H * W * 8 bytes for the z-buffer of the
    splat path.  If the allocation fails the batch is halved, and the last resort is the splat path's small workspace.
    return_parts: (scores, inter, nproj, nimg).  splat=True: the z-buffer splat path on purpose (its small workspace selects it in
    pcl_hist_trim_scores_images_sets; the tests compare the two renderers bit for bit)."""
    _unweighted(cloud, "hist_trim_scores")
    trans, rot = _dev(trans).reshape(1, -1, 3), _dev(rot).reshape(1, -1, 3)
    scores, inter, nproj, nimg = _hist_scores("hist_trim_scores", [_dev(img)], cloud, trans, rot, num_split_h, num_split_w, splat, batch=max(1, batch))
    return (scores[0], inter, nproj, nimg[0]) if return_parts else scores[0]


def hist_trim_scores_images(imgs, cloud, trans, rot, num_split_h, num_split_w, splat=False):
    """hist_trim_scores for several query images of one room in ONE set of launches: imgs = list of I (H, W, 3) float GPU images of
    one size, trans / rot (I, K, 3): image i's K candidates.  -> (I, K) scores, row i what hist_trim_scores(imgs[i], ...) returns
    (bit for bit: same keys, same integer counts, one carry-over chain per image).  Images go through in groups that keep the
    point lists within ~8 GB.  A cloud with colour sets (Cloud.with_color_sets, one per image): image i's candidates are rendered
    with set i, all images in one call.  splat=True: the z-buffer splat path on purpose (its small workspace selects it, as
    hist_trim_scores' flag), on either kind of cloud."""
    _unweighted(cloud, "hist_trim_scores_images")
    imgs = [_dev(im) for im in imgs]
    trans, rot = _dev(trans), _dev(rot)
    I, (H, W) = int(trans.shape[0]), (int(imgs[0].shape[0]), int(imgs[0].shape[1]))
    if len(imgs) != I or any(tuple(im.shape) != (H, W, 3) or not im.is_contiguous() for im in imgs):
        raise ValueError("hist_trim_scores_images: one contiguous (H, W, 3) image per row of candidates, all of one size")
    if cloud.color_sets > 1 and (cloud.color_sets != I or I > HIST_MAX_IMAGES):
        raise ValueError("a cloud of %d colour sets for %d images (at most %d per call)" % (cloud.color_sets, I, HIST_MAX_IMAGES))
    return _hist_scores("hist_trim_scores_images", imgs, cloud, trans, rot, num_split_h, num_split_w, splat)[0]


def _score_cloud(cloud, who):
    _unweighted(cloud, who)
    if cloud.color_sets > 1:
        raise ValueError("%s: a cloud of colour sets is not taken (one colour set, as the histogram parts it reads)" % who)


def score_maps(cloud, trans, rot, H, W, num_split_h, num_split_w, inter, nproj, nimg, packed=False):
    """(score3d (N,), count3d (N,) int32, score2d (nblk,), count2d (nblk,) int32) from the parts of hist_trim_scores(..., return_parts=True)
    for exactly these K poses and this split (pcl_score_maps, include/piccolo_hip.h): per scored image block the mean of `inter` over the
    poses whose block is valid (nproj > 0 and nimg > 0), per point the mean over the poses of the intersection of the block its centre
    pixel falls into; -1 and count 0 where nothing voted.  The 3D map is in the order of the cloud's xyz rows, packed=True: in packed
    order.  Two launches, no host synchronisation."""
    lib = _lib.load()
    _score_cloud(cloud, "score_maps")
    trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
    K, nblk = int(trans.shape[0]), (int(num_split_h) - 2) * int(num_split_w)
    inter, nproj, nimg = _dev(inter), _dev(nproj, torch.int32), _dev(nimg, torch.int32)
    nws = lib.pcl_score_maps_workspace_bytes(cloud.n, K, int(num_split_h), int(num_split_w))
    if nws == 0 or rot.shape[0] != K or int(H) // int(num_split_h) <= 0 or int(W) // int(num_split_w) <= 0:
        raise ValueError("score_maps: K >= 1 poses, num_split_h >= 3, num_split_w >= 1 and blocks of at least one pixel")
    if inter.numel() != K * nblk or nproj.numel() != K * nblk or nimg.numel() != nblk:
        raise ValueError("score_maps: inter / nproj must be (K, nblk) and nimg (nblk,) for these poses and this split")
    dev = cloud.data.device
    score3d, count3d = torch.empty(cloud.n, dtype=F32, device=dev), torch.empty(cloud.n, dtype=torch.int32, device=dev)
    score2d, count2d = torch.empty(nblk, dtype=F32, device=dev), torch.empty(nblk, dtype=torch.int32, device=dev)
    ws = _bytes(nws)
    _checked("pcl_score_maps", _ptr(cloud.data), cloud.n, _ptr(trans), _ptr(rot), K, int(H), int(W), int(num_split_h), int(num_split_w), _ptr(inter),
             _ptr(nproj), _ptr(nimg), None if packed else _ptr(cloud.order), _ptr(score3d), _ptr(count3d), _ptr(score2d), _ptr(count2d), _ptr(ws), nws,
             _stream())
    return score3d, count3d, score2d, count2d


def score_weight_plane(n, score_packed, count_packed, floor=0.0, min_count=1, plane=None):
    """(plane, range) from a 3D score map of n points in any one point order (pcl_score_weights): range = (lo, hi, voted) on the GPU, the
    smallest and largest score over the `voted` points with at least min_count votes; plane (pcl_cloud_stride(n) floats, what
    Cloud.weighted_view takes for a map in packed order) = floor + (1 - floor) (s - lo) / (hi - lo) for such a point, 1 for a point with
    fewer votes and for every point when nothing voted or hi == lo; padding 0.  plane: a tensor to write into."""
    lib = _lib.load()
    floor, min_count = float(floor), int(min_count)
    if not (0.0 <= floor < 1.0):
        raise ValueError("score_weight_plane: floor must be in [0, 1), got %r" % (floor,))
    if min_count < 1:
        raise ValueError("score_weight_plane: min_count must be at least 1, got %r" % (min_count,))
    score, count = _dev(score_packed), _dev(count_packed, torch.int32)
    nws = lib.pcl_score_weights_workspace_bytes(int(n))
    if nws == 0 or score.dim() != 1 or score.numel() != n or count.dim() != 1 or count.numel() != n:
        raise ValueError("score_weight_plane: one score and one count per point, (N,)")
    stride = lib.pcl_cloud_stride(n)
    if plane is None:
        plane = torch.empty(stride, dtype=F32, device=score.device)
    elif not (plane.is_cuda and plane.dtype == F32 and plane.is_contiguous() and plane.numel() == stride):
        raise ValueError("score_weight_plane: plane must be a contiguous float32 GPU tensor of pcl_cloud_stride(n) entries")
    rng = torch.empty(3, dtype=F32, device=score.device)
    ws = _bytes(nws)
    _checked("pcl_score_weights", _ptr(score), _ptr(count), int(n), min_count, floor, _ptr(plane), _ptr(rng), _ptr(ws), nws, _stream())
    return plane, rng


_VOXEL_BAD = ((1, "a NaN or infinite value"), (2, "a cell outside [-2^20, 2^20): the voxel is too small for the cloud's extent"),
              (4, "a magnitude of 32768 or more"))


def _voxel_bad(what, word):
    """ValueError naming every bit of a voxel call's bad set"""
    word = int(word)
    if word:
        raise ValueError("%s: %s" % (what, "; ".join(text for bit, text in _VOXEL_BAD if word & bit)))


def voxel_size(voxel, what="voxel"):
    """`voxel` as a float; ValueError unless it is a positive finite number.  Host only."""
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float)) or not (0.0 < float(voxel) < float("inf")):
        raise ValueError("%s %r: a positive finite number" % (what, voxel))
    return float(voxel)


def density_cap(cap, what="cap"):
    """`cap` as an int; ValueError unless it is an int >= 1.  Host only."""
    if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1:
        raise ValueError("%s %r: an int >= 1" % (what, cap))
    return int(cap)


class VoxelGrid:
    """The voxel grid of a cloud (pcl_voxel_grid; the rules: include/piccolo_hip.h): per axis
    cell = floor((double)x / voxel), the origin at 0, voxels numbered in the order in which xyz's rows first reach them.
      n, nvoxels     points, occupied voxels
      cell           (N,) int32: the voxel of every point, in the order of xyz's rows (never the packed cloud's Morton order)
      count, first   (V,) int32 / int64: a voxel's points and its lowest point index (strictly increasing with the voxel id)
    The call runs EAGERLY and ends with one 8-byte D2H read (the voxel count, which sizes the outputs, and the bad set): it does not belong
    inside a captured graph.  ValueError: an empty cloud, a voxel that is not a positive finite number, a NaN or infinite coordinate, a
    cell outside [-2^20, 2^20), a coordinate of magnitude 32768 or more.
    ws / buffers: a workspace of at least pcl_voxel_workspace_bytes(n) bytes and (count, first) buffers of N entries to use instead of fresh
    ones (count and first are then views of them; entries at and beyond nvoxels are left as they were)."""

    def __init__(self, xyz, voxel, ws=None, buffers=None):
        lib = _lib.load()
        self.voxel = voxel_size(voxel)
        if not torch.is_tensor(xyz):
            xyz = torch.as_tensor(xyz)
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError("xyz must be (N, 3)")
        self.n = int(xyz.shape[0])
        if self.n <= 0:
            raise ValueError("empty point cloud")
        xyz = _dev(xyz)
        nws = lib.pcl_voxel_workspace_bytes(self.n)
        if nws == 0:
            raise ValueError("VoxelGrid: %d points are more than a cloud holds" % self.n)
        ws = _voxel_ws(ws, nws)
        dev = xyz.device
        if buffers is None:
            count, first = torch.empty(self.n, dtype=torch.int32, device=dev), torch.empty(self.n, dtype=torch.int64, device=dev)
        else:
            count, first = buffers
            if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.numel() == self.n and first.is_cuda
                    and first.dtype == torch.int64 and first.is_contiguous() and first.numel() == self.n):
                raise ValueError("VoxelGrid: buffers must be contiguous GPU tensors (int32 count, int64 first) of N entries")
        self.cell = torch.empty(self.n, dtype=torch.int32, device=dev)
        words = torch.empty(2, dtype=torch.int32, device=dev)                     # (nvoxels, bad)
        _checked("pcl_voxel_grid", _ptr(xyz), self.n, self.voxel, _ptr(self.cell), _ptr(count), _ptr(first), _ptr(words), ctypes.c_void_p(words.data_ptr() + 4),
                 _ptr(ws), nws, _stream())
        nvoxels, bad = (int(v) for v in words.tolist())
        _voxel_bad("VoxelGrid: xyz holds", bad)
        self.nvoxels = nvoxels
        self.count, self.first = count[:nvoxels], first[:nvoxels]
        if buffers is None:                                                       # (keep V entries, not N)
            self.count, self.first = self.count.clone(), self.first.clone()
        self.xyz = xyz

    def centroids(self, rgb, ws=None):
        """(xyz', rgb'), (V, 3) float32 each in voxel-id order: per voxel the mean of its points' coordinates and colours over exact int64
        sums of llrint(a * 65536) — the same bits whatever the launch shape (pcl_voxel_centroids).  Eager, one 4-byte D2H read (the bad
        set).  ValueError: rgb that is not (N, 3), a NaN or infinite colour, a colour of magnitude 32768 or more."""
        lib = _lib.load()
        if not torch.is_tensor(rgb) or rgb.dim() != 2 or tuple(rgb.shape) != (self.n, 3):
            raise ValueError("rgb must be one (N, 3) tensor")
        rgb = _dev(rgb)
        nws = lib.pcl_voxel_workspace_bytes(self.n)
        ws = _voxel_ws(ws, nws)
        dev = self.xyz.device
        xyz_out, rgb_out = torch.empty(self.nvoxels, 3, dtype=F32, device=dev), torch.empty(self.nvoxels, 3, dtype=F32, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        _checked("pcl_voxel_centroids", _ptr(self.xyz), _ptr(rgb), self.n, _ptr(self.cell), _ptr(self.count), self.nvoxels, _ptr(xyz_out), _ptr(rgb_out),
                 _ptr(bad), _ptr(ws), nws, _stream())
        _voxel_bad("VoxelGrid.centroids: the cloud holds", bad.item())
        return xyz_out, rgb_out

    def weights(self, cap=1):
        """(N,) float32 density weights in the order of xyz's rows: 1 where the point's voxel holds at most `cap` points, else
        (float)((double)cap / count) (pcl_density_weights) — with cap = 1 every occupied voxel has total weight 1."""
        cap = density_cap(cap)
        w = torch.empty(self.n, dtype=F32, device=self.cell.device)
        _checked("pcl_density_weights", _ptr(self.cell), _ptr(self.count), self.n, self.nvoxels, cap, _ptr(w), _stream())
        return w

    def moments(self, out=None):
        """(V, 9) int64 in voxel-id order: per voxel the exact sums S1 = sum d (3) and S2 = sum d_a d_b (xx, xy, xz, yy, yz, zz) of
        d = llrint(x * 65536) - llrint(x_first * 65536), the offsets from the voxel's first point (pcl_voxel_moments): integers, the same
        bits for any launch shape.  (Which point is a voxel's first depends on the order of xyz's rows: another order gives other moments
        and, exactly, the same scatter matrix count S2 - S1 S1^T, so the same normals.)  Eager, one 4-byte D2H read (the bad set).  ValueError: a voxel above 2 m (the sums' range rule,
        include/piccolo_hip.h).  out: a contiguous (V, 9) int64 GPU tensor to write into."""
        if self.voxel > ALIGN_MAX_VOXEL:
            raise ValueError("VoxelGrid.moments: voxel %r: at most %g m (the exact sums' range)" % (self.voxel, ALIGN_MAX_VOXEL))
        dev = self.xyz.device
        if out is None:
            out = torch.empty(self.nvoxels, 9, dtype=torch.int64, device=dev)
        elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (self.nvoxels, 9)):
            raise ValueError("VoxelGrid.moments: out must be a contiguous (V, 9) int64 GPU tensor")
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        _checked("pcl_voxel_moments", _ptr(self.xyz), self.n, self.voxel, _ptr(self.cell), _ptr(self.first), self.nvoxels, _ptr(out), _ptr(bad), _stream())
        _voxel_bad("VoxelGrid.moments: xyz holds", bad.item())
        return out

    def normals(self, min_count=8, return_eig=False):
        """(normal (V, 3), planarity (V,)[, eig (V, 3)]) float32 in voxel-id order, from moments(): the plane fit of every voxel with at
        least min_count points (pcl_voxel_normals) — the unit eigenvector of the covariance's smallest eigenvalue, signed so that its
        component of largest magnitude is positive; planarity = (l1 - l0) / l2; eig = (l0, l1, l2) in m^2.  A voxel with fewer points, or
        all of whose points coincide, gets zeros.  ValueError: min_count that is not an int >= 3."""
        return voxel_normals_of(self.moments(), self.count, min_count, return_eig)


ALIGN_MAX_VOXEL = 2.0


def align_min_count(min_count, what="min_count"):
    """`min_count` as an int; ValueError unless it is an int >= 3 (a plane needs three points).  Host only."""
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 3:
        raise ValueError("%s %r: an int >= 3" % (what, min_count))
    return int(min_count)


def align_max_tilt(max_tilt, what="max_tilt"):
    """`max_tilt` in degrees as a float; ValueError unless it is a number in (0, 45].  Host only."""
    if isinstance(max_tilt, bool) or not isinstance(max_tilt, (int, float)) or not (0.0 < float(max_tilt) <= 45.0):
        raise ValueError("%s %r: degrees in (0, 45]" % (what, max_tilt))
    return float(max_tilt)


def voxel_normals_of(moments, count, min_count=8, return_eig=False):
    """VoxelGrid.normals on moments and counts the caller holds: (V, 9) int64 and (V,) int32 GPU tensors."""
    min_count = align_min_count(min_count)
    if not (torch.is_tensor(moments) and moments.is_cuda and moments.dtype == torch.int64 and moments.is_contiguous() and moments.dim() == 2
            and moments.shape[1] == 9 and moments.shape[0] > 0):
        raise ValueError("moments must be a contiguous (V, 9) int64 GPU tensor")
    V = int(moments.shape[0])
    count = _dev(count, torch.int32)
    if tuple(count.shape) != (V,):
        raise ValueError("count must be (V,), one entry per row of moments")
    dev = moments.device
    normal, planarity = torch.empty(V, 3, dtype=F32, device=dev), torch.empty(V, dtype=F32, device=dev)
    eig = torch.empty(V, 3, dtype=F32, device=dev) if return_eig else None
    _checked("pcl_voxel_normals", _ptr(moments), _ptr(count), V, min_count, _ptr(normal), _ptr(planarity), _ptr(eig), _stream())
    return (normal, planarity, eig) if return_eig else (normal, planarity)


def align_vote(normal, planarity, count, max_tilt=40.0, yaw=False, ws=None):
    """The up direction (and with yaw the wall direction) of a cloud from its voxels' normals (V, 3), planarities (V,) and counts (V,)
    (pcl_align_vote; the recipe: include/piccolo_hip.h).  Eager, one D2H copy of the 168-byte record.  -> a dict:
      up (3,), rot (3, 3)   float64 numpy: the up vector in the cloud's frame, and align_rot — x_aligned = rot @ x
      tilt, yaw             radians: atan2 of the record's (sin, cos) pairs, taken here on the host; yaw in (-pi/4, pi/4]
      cos_tilt, sin_tilt, cos_yaw, sin_yaw    the pairs themselves
      weights               (up bins, last cone round, wall bins, wall mean): the integer weight each stage kept
      status                0; 1: no voxel inside the tilt cone (rot is the identity); 2: no wall normals (yaw 0)
    ws: a contiguous uint8 GPU workspace of at least pcl_align_workspace_bytes(V) bytes to use instead of a fresh one (DESIGN.md section 2b's
    contract for it — the same bits whatever it held, no write outside the queried bytes — is pinned by tests/test_align.py).
    ValueError: max_tilt outside (0, 45] degrees, yaw that is not a bool, shapes that do not agree, a workspace that is too small."""
    import math
    max_tilt = align_max_tilt(max_tilt)
    if not isinstance(yaw, bool):
        raise ValueError("yaw %r: a bool" % (yaw,))
    if not torch.is_tensor(normal) or normal.dim() != 2 or normal.shape[1] != 3 or normal.shape[0] <= 0:
        raise ValueError("normal must be (V, 3)")
    V = int(normal.shape[0])
    normal, planarity, count = _dev(normal), _dev(planarity), _dev(count, torch.int32)
    if tuple(planarity.shape) != (V,) or tuple(count.shape) != (V,):
        raise ValueError("planarity and count must be (V,), one entry per normal")
    lib = _lib.load()
    nws = lib.pcl_align_workspace_bytes(V)
    if ws is None:
        ws = torch.empty(int(nws), dtype=torch.uint8, device=normal.device)
    elif not (torch.is_tensor(ws) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nws):
        raise ValueError("ws must be a contiguous uint8 GPU tensor of at least pcl_align_workspace_bytes(V) = %d bytes" % nws)
    out = torch.empty(_lib.ALIGN_OUT_WORDS, dtype=torch.float64, device=normal.device)
    params = _lib.AlignParams(max_tilt, int(yaw), 0)
    _checked("pcl_align_vote", _ptr(normal), _ptr(planarity), _ptr(count), V, ctypes.byref(params), _ptr(out), _ptr(ws), nws, _stream())
    rec = out.cpu()
    d, w = rec[:16].numpy(), rec[16:].view(torch.int64).tolist()
    return {"up": d[0:3].copy(), "rot": d[3:12].reshape(3, 3).copy(), "cos_tilt": float(d[12]), "sin_tilt": float(d[13]), "cos_yaw": float(d[14]),
            "sin_yaw": float(d[15]), "tilt": math.atan2(float(d[13]), float(d[12])), "yaw": math.atan2(float(d[15]), float(d[14])),
            "weights": tuple(w[:4]), "status": int(w[4])}


def align_transform_cloud(xyz, rot, trans):
    """(N, 3) float32: rot (x - trans) per point, rot a (3, 3) matrix and trans 3 values (pcl_align_transform_cloud: fp32, d = x - trans,
    out_r = (R_r0 d_0 + R_r1 d_1) + R_r2 d_2, no contraction).  The reference's `np.matmul(align_rot, xyz.T - align_trans).T`
    (localize.py:157) with stated bits.  (transform_cloud is the POSE form: a translation and yaw / pitch / roll.)"""
    if not torch.is_tensor(xyz):
        xyz = torch.as_tensor(xyz)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] <= 0:
        raise ValueError("xyz must be (N, 3) with at least one point")
    x = _dev(xyz)
    r, t = _dev(torch.as_tensor(rot)), _dev(torch.as_tensor(trans))
    if r.numel() != 9 or (r.dim() == 2 and tuple(r.shape) != (3, 3)):
        raise ValueError("rot must be a (3, 3) matrix")
    if t.numel() != 3:
        raise ValueError("trans must hold 3 values")
    out = torch.empty_like(x)
    _checked("pcl_align_transform_cloud", _ptr(x), int(x.shape[0]), _ptr(r), _ptr(t), _ptr(out), _stream())
    return out


def _voxel_ws(ws, nws):
    """the caller's workspace, checked, or a fresh one (DESIGN.md section 2b's contract for it — results independent of its contents, no
    write outside the queried bytes — is pinned by tests/test_voxel.py with the same three fill words, on a workspace the test brings)"""
    if ws is None:
        return torch.empty(max(int(nws), 16), dtype=torch.uint8, device=device())
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nws):
        raise ValueError("ws must be a contiguous uint8 GPU tensor of at least pcl_voxel_workspace_bytes(n) = %d bytes" % nws)
    return ws


def depth_mask(cloud, trans, rot, resolution, tau=None, stride=1):
    """(B, n) uint8 GPU tensor in PACKED point order: scatter-min visibility of every point for every pose on a z-buffer grid of
    `resolution` = (depth_h, depth_w) cells (the DEPTH grid — see default_depth — not the panorama's size) built from every
    stride-th packed point; tau None: the rule's tolerance for that grid."""
    lib = _lib.load()
    trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
    B, (H, W) = int(trans.shape[0]), (int(resolution[0]), int(resolution[1]))
    if tau is None:
        tau = depth_tau_rule(H)
    vis = torch.empty(B, cloud.n, dtype=torch.uint8, device=trans.device)
    nws = lib.pcl_depth_workspace_bytes(B, H, W)
    ws = _bytes(nws)
    _checked("pcl_depth_mask", _ptr(cloud.data), cloud.n, _ptr(trans), _ptr(rot), B, H, W, float(tau), int(stride), _ptr(vis), _ptr(ws), nws, _stream())
    return vis


class ColorTemplate:
    """The point colours sorted per channel (3, n): what color_match needs from the cloud, built once per cloud."""

    def __init__(self, rgb):
        lib = _lib.load()
        rgb = _dev(rgb).reshape(-1, 3)
        self.n = int(rgb.shape[0])
        self.data = torch.empty(3, self.n, dtype=F32, device=rgb.device)
        nws = lib.pcl_color_template_workspace_bytes(self.n)
        ws = _bytes(nws)
        _checked("pcl_color_template_build", _ptr(rgb), self.n, _ptr(self.data), _ptr(ws), nws, _stream())


def color_match(img, template):
    """color_utils.color_match (color_utils.py:146-234) on the GPU: img (H,W,3) with levels k/255 -> matched (H,W,3).
    `template` is a ColorTemplate of the point colours."""
    lib = _lib.load()
    known = _known_levels(img)
    img = _dev(img)
    H, W = int(img.shape[0]), int(img.shape[1])
    out = torch.empty_like(img)
    flag = torch.zeros(1, dtype=torch.int32, device=img.device)
    nws = lib.pcl_color_workspace_bytes()
    ws = _bytes(nws)
    _checked("pcl_color_match", _ptr(img), H, W, _ptr(template.data), template.n, _ptr(out), _ptr(flag), _ptr(ws), nws, _stream())
    if not known and int(flag.item()):
        raise ValueError("color_match: the panorama must hold levels k/255 (an image file's uint8 / 255); "
                         "found a non-black pixel channel in between")
    return out


def color_mod(img, rgb, num_bins=256):
    """color_utils.color_mod (color_utils.py:7-65) on the GPU: -> (img (H,W,3), rgb (n,3)) after joint luma equalisation."""
    lib = _lib.load()
    img, rgb = _dev(img), _dev(rgb).reshape(-1, 3)
    H, W = int(img.shape[0]), int(img.shape[1])
    out_img, out_rgb = torch.empty_like(img), torch.empty_like(rgb)
    nws = lib.pcl_color_workspace_bytes()
    ws = _bytes(nws)
    _checked("pcl_color_mod", _ptr(img), H, W, _ptr(rgb), int(rgb.shape[0]), int(num_bins), _ptr(out_img), _ptr(out_rgb), _ptr(ws), nws, _stream())
    return out_img, out_rgb


def histogram(img, mask, channels, normalize=True, eps=0.0):
    """color_utils.histogram on the GPU.  One image (color_utils.py:68-103), (H,W,3) / (H,W): flat float histogram of c0*c1*c2 bins.
    A batch (color_utils.py:103-117), (B,H,W,3) / (B,H,W) -> (B, c0*c1*c2): the maximum of the whole batch decides whether the colours
    are scaled by 255, as the reference's one `tgt_img.max() <= 1` does (the caller passes the batched form's eps)."""
    lib = _lib.load()
    B = int(img.shape[0]) if len(img.shape) == 4 else 0             # 0: the unbatched form
    img = _dev(img).reshape(-1, 3)
    mask = _dev(mask != 0, torch.uint8).reshape(-1)
    c0, c1, c2 = (int(c) for c in channels)
    nws = lib.pcl_histogram_batch_workspace_bytes(B, c0, c1, c2) if B else lib.pcl_histogram_workspace_bytes(c0, c1, c2)
    if nws == 0:
        raise ValueError("histogram: bad bin counts %r (or batch size %d)" % (channels, B))
    ws = _bytes(nws)
    hist = torch.empty(max(B, 1) * c0 * c1 * c2, dtype=F32, device=img.device)
    if B:
        _checked("pcl_histogram_batch", _ptr(img), _ptr(mask), B, int(img.shape[0]) // B, c0, c1, c2, int(bool(normalize)), float(eps), _ptr(hist), _ptr(ws),
                 nws, _stream())
        return hist.reshape(B, -1)
    _checked("pcl_histogram", _ptr(img), _ptr(mask), int(img.shape[0]), c0, c1, c2, int(bool(normalize)), float(eps), _ptr(hist), _ptr(ws), nws, _stream())
    return hist


def histogram_intersection(h1, h2):
    """(B, nbins) x (B, nbins) -> (B,) sums of element-wise minima (color_utils.py:122-144)."""
    h1, h2 = _dev(h1), _dev(h2)
    B, nbins = int(h1.shape[0]), int(h1.shape[1])
    out = torch.empty(B, dtype=F32, device=h1.device)
    _checked("pcl_histogram_intersection", _ptr(h1), _ptr(h2), B, nbins, _ptr(out), _stream())
    return out


def quantile_box(xyz, q):
    """(6,) GPU tensor: x_lo, x_hi, y_lo, y_hi, z_lo, z_hi — utils.py:208-229 on the three columns."""
    lib = _lib.load()
    xyz = _dev(xyz)
    box = torch.empty(6, dtype=F32, device=xyz.device)
    ws = _bytes(lib.pcl_quantile_workspace_bytes())
    _checked("pcl_quantile_box", _ptr(xyz), int(xyz.shape[0]), float(q), _ptr(box), _ptr(ws), _stream())
    return box


def _gd_hyper(lr, patience, factor, batch_mode, fuse, depth=None, color_sets=0):
    """The hyper-parameter struct of every GD engine.  depth: None, or the mask's (depth_h, depth_w, tau, occluder stride); fuse False: always
    the two-launch form; a negative int: pcl_gd_hyper.fuse as it is (-2: two launches on the caller's stream alone, -3: two half-chains
    on two streams whenever there are two pose groups — what the tests of the split compare)."""
    dh, dw, tau, st = depth or (0, 0, 0.0, 0)
    if fuse is None or fuse is True:
        fz = 0
    elif fuse is False:
        fz = -1
    elif isinstance(fuse, int) and -3 <= fuse <= 0:
        fz = int(fuse)
    else:
        raise ValueError("fuse: None, True, False or pcl_gd_hyper.fuse's 0, -1, -2, -3, not %r" % (fuse,))
    return _lib.GdHyper(float(lr), float(factor), int(patience), _lib.GD_BATCH if batch_mode else _lib.GD_SEQUENTIAL, 1 if depth else 0, float(tau),
                        int(dh), int(dw), int(st), fz, 0, int(color_sets))


class _GdEngine:
    """What the GD engines share: a state of self.B candidates (self.state), a run(num_iter) that neither allocates nor synchronises, and
    self.pano, the panorama whose size and texel format every panorama of the chain has.  A class says how its candidates split into groups
    (_groups, _GROUP), what a smaller engine takes over as it is (_INHERITED) and how large a workspace it needs (_workspace_bytes)."""

    _chain = None                   # an inner engine whose hyper-parameters, state and workspace are this object's (GradientDescent's)

    def _size(self, B):
        self.B = B

    def _allocate(self, smaller=False):
        """the state and the workspace of self.B candidates under self.hyper; the class says how large (_workspace_bytes) and what 0 means"""
        self.state = _bytes(_lib.load().pcl_gd_state_bytes(self.B))
        self.ws_bytes = self._workspace_bytes()
        if self.ws_bytes == 0:
            raise _lib.PiccoloHipError(self._refusal(smaller))
        self.ws = _bytes(self.ws_bytes)

    def _share(self, inner):
        self._chain, self.hyper, self.state, self.ws, self.ws_bytes = inner, inner.hyper, inner.state, inner.ws, inner.ws_bytes

    def _smaller(self, keep):
        """An engine of the same class, clouds, panorama, boxes and hyper-parameters with `keep` candidates per group, its state not yet
        written: the attributes _INHERITED names, a copy of the hyper-parameters, buffers of its own.  Nothing tied to THIS engine's buffers
        goes along — captured graphs, robust planes, a cached engine's private clouds; prune_into hands over the named panoramas."""
        groups = self._groups()
        if self.B % groups or not 1 <= keep <= self.B // groups:
            raise ValueError("pruned: keep %d of %d candidates per %s" % (keep, self.B // groups, self._GROUP))
        g = type(self).__new__(type(self))
        for name in self._INHERITED:
            setattr(g, name, getattr(self, name))
        g._size(groups * keep)
        if self._chain is not None:
            g._share(self._chain._smaller(keep))
        else:
            g.hyper = _copy_hyper(self.hyper)
            g._allocate(smaller=True)
        return g

    def _leaf_check(self, who, *leaves):
        for t in leaves:
            if t is not None and not (t.is_cuda and t.dtype == F32 and t.is_contiguous() and t.numel() == 3 * self.B):
                raise ValueError("%s: leaf buffers must be contiguous float32 GPU tensors of B x 3" % who)

    def run_graph(self, num_iter):
        """Same as run(num_iter) but the 2 * num_iter launches are captured into one hipGraph and replayed: the host
        enqueues one graph instead of 200 kernels per refinement (pcl_gd_run neither allocates nor synchronises, so it
        is capture-safe).  The instantiated graph is cached per num_iter and _graph_key() — what else the captured launches
        depend on: a graph captured for an unweighted segment is never replayed for a weighted one; replaying it continues
        from the current state, exactly like calling run() again."""
        cache = self.__dict__.setdefault("_graphs", {})
        key = (num_iter,) + tuple(self._graph_key())
        g = cache.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream(device=self.state.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    self.run(num_iter)
            torch.cuda.current_stream().wait_stream(side)
            cache[key] = g
            # capture does not execute: fall through to the first replay
        g.replay()

    def _graph_key(self):
        """what, besides num_iter, a captured run() depends on (GradientDescent: the weight plane it reads)"""
        return ()

    def _name_panos(self, panos):
        """The pose records of candidates [i * B / I, (i + 1) * B / I) name panos[i] (I Pano objects of the size / texel format of self.pano):
        nothing is copied to the device, the addresses are kernel arguments (pcl_gd_set_pano_groups)."""
        I = len(panos)
        if I <= 0 or self.B % I:
            raise ValueError("set_pano_groups: %d candidates do not split into %d images" % (self.B, I))
        _same_texels(panos, self.pano)
        self._panos = list(panos)                      # keep them alive
        arr = (ctypes.c_uint64 * I)(*[p.data.data_ptr() for p in panos])
        _checked("pcl_gd_set_pano_groups", _ptr(self.state), arr, I, self.B // I, _stream())

    def winners(self, groups, leaf_trans=None, leaf_rot=None):
        """(groups, 16) GPU tensor, per group of B / groups candidates the one omniloc_batch returns (omniloc.py:271-277):
        post-step t (3), R (9), last loss, yaw / pitch / roll.  leaf_trans / leaf_rot: contiguous float32 GPU tensors of B x 3
        that receive every candidate's leaf parameters (the reference optimises the caller's rows in place)."""
        if groups <= 0 or self.B % groups:
            raise ValueError("winner: %d candidates do not split into %d images" % (self.B, groups))
        out = torch.empty(groups, 16, dtype=F32, device=self.state.device)
        self._leaf_check("winner", leaf_trans, leaf_rot)
        _checked("pcl_gd_winner", _ptr(self.state), groups, self.B // groups, _ptr(out), _ptr(leaf_trans), _ptr(leaf_rot), _stream())
        return out

    def result(self):
        """(B, 16): fwd t(3), fwd ypr(3), leaf t(3), leaf ypr(3), last loss, lr, scheduler num_bad_epochs, scheduler best."""
        out = torch.empty(self.B, _lib.GD_RESULT_STRIDE, dtype=F32, device=self.state.device)
        _checked("pcl_gd_result", _ptr(self.state), self.B, _ptr(out), _stream())
        return out

    def pruned(self, keep, leaf_trans=None, leaf_rot=None):
        """-> (engine, survivors): an engine of the same class over the same clouds, panoramas, boxes and hyper-parameters with the `keep`
        best candidates of every group (an image; a (room, image)) by their last loss, and the survivors' indices inside their groups
        ((groups * keep,) int32 on the device, original order).  The smaller engine's state is pcl_gd_prune's output — the survivors'
        complete optimiser state, pose records, panoramas and colour sets — and it has a workspace of its own for the smaller plan; run it
        to continue the chain.  leaf_trans / leaf_rot: as for winners(), every candidate of THIS engine.  No synchronisation, no D2H."""
        child = self._smaller(int(keep))
        return child, self.prune_into(child, leaf_trans, leaf_rot)

    def prune_into(self, child, leaf_trans=None, leaf_rot=None):
        """pruned() into an engine that exists (the same class, clouds and groups, fewer candidates per group: a cached one whose captured
        graph is to be replayed): its state is overwritten.  -> survivors"""
        groups = self._groups()
        if type(child) is not type(self) or child is self or child.B <= 0 or child.B % groups or child.B > self.B or not self._same_problem(child):
            raise ValueError("prune: the smaller engine must be one of the same class, clouds and groups with at most as many candidates")
        self._leaf_check("prune", leaf_trans, leaf_rot)
        if self.B // groups > _lib.GD_PRUNE_MAX:
            raise ValueError("prune: at most %d candidates per group" % _lib.GD_PRUNE_MAX)
        survivors = torch.empty(child.B, dtype=torch.int32, device=self.state.device)
        _checked("pcl_gd_prune", _ptr(self.state), groups, self.B // groups, child.B // groups, _ptr(child.state), _ptr(survivors), _ptr(leaf_trans),
                 _ptr(leaf_rot), _stream())
        # the survivors' records name the parent's panoramas: keep them alive, and the mapping hint with them
        child.hyper.images = self.hyper.images
        for name in ("_panos", "_pano_table"):
            if name in self.__dict__:
                setattr(child, name, self.__dict__[name])
        return survivors


def _copy_hyper(h):
    c = _lib.GdHyper()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(h), ctypes.sizeof(c))
    return c


class GradientDescent(_GdEngine):
    """On-device GD refinement of B candidates (Adam + ReduceLROnPlateau + clamp), pcl_gd_* of the C ABI."""

    _INHERITED, _GROUP = ("cloud", "pano", "box"), "image"
    weight_sets, _robust = 0, None  # (a smaller engine's: no weight sets, no plane of its own)

    def __init__(self, cloud, pano, trans, rot, box, lr=0.1, patience=5, factor=0.9, batch_mode=True, depth_mask=False,
                 depth_tau=None, depth_res=None, depth_stride=None, fuse=None, weight_sets=0):
        """fuse None: pcl_gd_plan's rule (one launch per iteration for launches whose blocks are all resident); False: always the
        two-launch form (bit-identical; tests and measurements).
        weight_sets I >= 1: the candidates are I images of B / I (set_pano_groups names their panoramas) and the engine is the weight-set
        chain (pcl_gd_run_weight_sets): the single-image plan for all B candidates with shared colours too, pose records that name their
        image, and I weight planes of its own (self.weight_planes(), unused until robust_reweight or weight_planes_on) — image i's results are
        those of a GradientDescent over image i alone, bit for bit.  One colour set or I of them, no depth mask, a cloud without weights."""
        self.cloud, self.pano = cloud, pano
        trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
        self._size(int(trans.shape[0]))
        self.box = _dev(box).reshape(6)
        self.weight_sets, self._robust = int(weight_sets), None       # (_robust: _robust_buffers, once a re-weighting or a plane asks for them)
        if self.weight_sets:
            if self.weight_sets < 1 or self.B % self.weight_sets or depth_mask or cloud.weights is not None or \
                    cloud.color_sets not in (1, self.weight_sets):
                raise ValueError("GradientDescent: weight_sets=%d needs B (%d) candidates that split into that many images, one colour set or one "
                                 "per image, no depth mask and a cloud without weights" % (self.weight_sets, self.B))
        if cloud.weights is not None and depth_mask:
            raise ValueError("GradientDescent: per-point weights do not combine with the depth mask")
        if cloud.color_sets > 1 and self.B % cloud.color_sets:
            raise ValueError("GradientDescent: %d candidates over %d colour sets" % (self.B, cloud.color_sets))
        # colour sets under the depth mask: the depth-chain family with this cloud as its one room and a set per image; the engine's state,
        # workspace and hyper-parameters are this object's (the pose records name no panorama until set_pano_groups)
        if depth_mask and cloud.color_sets > 1:
            self._share(GradientDescentRoomsImages([(cloud, self.box)], [pano] * cloud.color_sets, trans, rot, lr, patience, factor, batch_mode, fuse,
                                                   True, depth_tau, depth_res, depth_stride, name_panos=False))
            return
        # a cloud of per-image colour sets (Cloud.with_color_sets): candidates [i * B / k, (i + 1) * B / k) read set i, and the chain runs
        # the single-image plan (pcl_gd_hyper.color_sets)
        self.hyper = _gd_hyper(lr, patience, factor, batch_mode, fuse, _depth_args(cloud.n, pano.H, pano.W, depth_res, depth_tau, depth_stride)
                               if depth_mask else None, cloud.color_sets)
        self._allocate()
        self.reset(trans, rot)

    def _workspace_bytes(self):
        if self.weight_sets:
            return _lib.load().pcl_gd_weight_sets_workspace_bytes(self.cloud.n, self.B, self.weight_sets, ctypes.byref(self.hyper))
        return _lib.load().pcl_gd_workspace_bytes(self.cloud.n, self.B, self.pano.H, self.pano.W, ctypes.byref(self.hyper))

    def _refusal(self, smaller):
        h = self.hyper
        return "pcl_gd_workspace_bytes: invalid arguments " + ("for %d candidates" % self.B if smaller else "(depth grid %dx%d?)" % (h.depth_h, h.depth_w))

    def run(self, num_iter, history=False, timer=None):
        if self._chain is not None:
            return self._chain.run(num_iter, history, timer)
        hist = torch.empty(num_iter, self.B, dtype=F32, device=self.state.device) if history else None
        weights = self._run_weights()
        if self.weight_sets:
            # (planes at a stable address, like the one plane below; None: the unweighted loss under the same single-image plan)
            _checked("pcl_gd_run_weight_sets", _ptr(self.cloud.data), _ptr(weights), self.weight_sets, self.cloud.n, _ptr(self.pano.data), self.pano.fmt,
                     self.pano.H, self.pano.W, _ptr(self.state), self.B, _ptr(self.box), ctypes.byref(self.hyper), int(num_iter), _ptr(hist), _ptr(self.ws),
                     self.ws_bytes, timer.handle if timer else None, _stream())
            return hist
        if weights is not None:
            # (the plane's address is the cloud's for good — Cloud.set_weights packs in place — so a captured graph reads the current weights)
            _checked("pcl_gd_run_weighted", _ptr(self.cloud.data), _ptr(weights), self.cloud.n, _ptr(self.pano.data), self.pano.fmt, self.pano.H, self.pano.W,
                     _ptr(self.state), self.B, _ptr(self.box), ctypes.byref(self.hyper), int(num_iter), _ptr(hist), _ptr(self.ws), self.ws_bytes,
                     timer.handle if timer else None, _stream())
            return hist
        _checked("pcl_gd_run", _ptr(self.cloud.data), self.cloud.n, _ptr(self.pano.data), self.pano.fmt, self.pano.H, self.pano.W, _ptr(self.state), self.B,
                 _ptr(self.box), ctypes.byref(self.hyper), int(num_iter), _ptr(hist), _ptr(self.ws), self.ws_bytes, timer.handle if timer else None, _stream())
        return hist

    def _run_weights(self):
        """the weight plane run() evaluates: the engine's own robust plane once robust_reweight has filled it, else the cloud's, else None"""
        return self._robust["plane"] if self._robust is not None and self._robust["on"] else self.cloud.weights

    def _graph_key(self):
        w = self._run_weights() if self._chain is None else None
        # (the panorama's size and texel format: run_pyramid's segments run one engine against several)
        return (0 if w is None else w.data_ptr(), self.weight_sets) + tuple(self.pano.texels)

    def _robust_buffers(self):
        """the engine's own plane(s), residual row(s), scale(s) and select workspace, at stable addresses: one per image of a weight-set engine"""
        if self._robust is None:
            lib, dev, I = _lib.load(), self.state.device, max(1, self.weight_sets)
            self._robust = {"on": False, "plane": torch.empty(I * lib.pcl_cloud_stride(self.cloud.n), dtype=F32, device=dev),
                            "row": torch.empty(I, self.cloud.n, dtype=F32, device=dev), "scale": torch.empty(2 * I, dtype=F32, device=dev),
                            "ws": _bytes(lib.pcl_robust_weights_rows_workspace_bytes(self.cloud.n, I))}
        return self._robust

    def weight_planes(self):
        """(I, pcl_cloud_stride(n)) view of a weight-set engine's planes, packed point order (what robust_reweight fills in place)"""
        if not self.weight_sets:
            raise ValueError("weight_planes: an engine made with weight_sets")
        return self._robust_buffers()["plane"].view(self.weight_sets, -1)

    def weight_planes_on(self, on=True):
        """run() evaluates the weighted loss with weight_planes() as they are (on) or the unweighted one (off): for planes a caller filled"""
        if not self.weight_sets:
            raise ValueError("weight_planes_on: an engine made with weight_sets")
        self._robust_buffers()["on"] = bool(on)

    # ---- robust re-weighting (cfg.robust_iters of omniloc_batch): the SAME state goes on under weights made from its own winner's residuals.
    def robust_clear(self):
        """back to the cloud's own weights (none, for a robust chain): what a new refinement on a cached engine starts with"""
        if self._robust is not None:
            self._robust["on"] = False

    def robust_reweight(self, kind="trunc", k=2.5):
        """pcl_gd_winner over the I = max(1, weight_sets) image groups -> the residuals at the poses that call reports (stride 16, packed, on
        the device; image i's panorama and colour set) -> pcl_robust_weights_rows into the engine's OWN I planes, in place at stable
        addresses; from here on run() evaluates the weighted loss with the state as it is.  Eight launches, nothing waits for the host.
        An engine made without weight_sets: one image, one colour set, no depth mask, a cloud without weights of its own.
        -> (plane, scale) of this re-weighting: `stride` floats and the device (s, M); a weight-set engine: (I, stride) and (I, 2)."""
        I = max(1, self.weight_sets)
        panos = self.__dict__.get("_panos") or [self.pano] * I
        if self.weight_sets:
            if len(panos) != I:
                raise ValueError("robust_reweight: %d panoramas named for %d images (set_pano_groups)" % (len(panos), I))
        else:
            if self._chain is not None or self.hyper.depth_mask or self.cloud.color_sets > 1:
                raise ValueError("robust_reweight: one colour set and no depth mask")
            if self.cloud.weights is not None:
                raise ValueError("robust_reweight: the cloud carries per-point weights of its own")
            if len({id(p) for p in panos}) > 1:
                raise ValueError("robust_reweight: the candidates of one image only (several: an engine made with weight_sets)")
            if kind not in ROBUST_KINDS:
                raise ValueError("robust_reweight: kind %r (one of %s)" % (kind, sorted(ROBUST_KINDS)))
            panos = panos[0]                           # (one Pano: pcl_point_residuals, as for any number of poses on one panorama)
        r = self._robust_buffers()
        who = "point_residuals_images_at_winners" if self.weight_sets else "point_residuals_at_winners"
        win = self.winners(I)
        _point_residuals(who, self.cloud, panos, *_winner_poses(win, who, I), win.device, True, r["row"])
        planes, scales = robust_planes(self.cloud.n, r["row"], kind, k, r["plane"].view(I, -1), r["scale"].view(I, 2), r["ws"])
        r["on"] = True
        return (planes, scales) if self.weight_sets else (r["plane"], r["scale"])

    def run_robust(self, num_iter, robust_iters, kind="trunc", k=2.5, history=False, graph=False):
        """The robust chain: unweighted up to robust_iters[0]; at every entry of robust_iters robust_reweight(kind, k), and the same state
        goes on weighted.  graph: every segment replays its captured graph (no history then).  The loss a segment reports is ITS loss: weighted
        after the first entry — also the last forward's that winners() / result() hand back.  Adam's moments and the plateau scheduler carry
        on across a switch; the scheduler's `best` then compares weighted with unweighted losses (it is not reset).  An engine made with
        weight_sets=I runs it for its I image groups at once: every image its own winner, residual row, scale and plane.  -> history or None"""
        iters = [int(i) for i in robust_iters]
        if not iters or any(not 0 < i < num_iter for i in iters) or any(b <= a for a, b in zip(iters, iters[1:])):
            raise ValueError("run_robust: robust_iters %r: strictly increasing iteration counts inside (0, %d)" % (iters, num_iter))
        self.robust_clear()
        hists, done = [], 0
        for end in iters + [int(num_iter)]:
            if done:
                self.robust_reweight(kind, k)
            if graph:
                self.run_graph(end - done)
            else:
                hists.append(self.run(end - done, history))
            done = end
        return torch.cat(hists) if history and not graph else None

    # ---- coarse-to-fine (cfg.pyramid_iters of omniloc_batch): the SAME state goes on against the next finer level of a panorama pyramid.
    def run_pyramid(self, pyramids, num_iter, iters, reset_plateau=False, history=False, graph=False):
        """The coarse-to-fine chain over `pyramids`, one PanoPyramid per image of the engine (1, or the I of set_pano_groups: candidates
        [i * B / I, (i + 1) * B / I) sample image i's levels).  iters = [i_1 < ... < i_L] strictly inside (0, num_iter), L the coarse levels
        used: iterations [0, i_1) run on level L, [i_1, i_2) on level L - 1, ..., [i_L, num_iter) on level 0.  At a switch the engine takes
        the next level's size and texel format for its launches and names that level's panoramas in the pose records; nothing else
        changes: Adam's moments, every candidate's lr and the step count ALWAYS carry on.  Without reset_plateau the plateau scheduler's
        `best` and its bad-epoch count carry on too — `best` then compares the losses of one level with those of another, as run_robust's
        compares weighted with unweighted ones (it is not reset); with reset_plateau pcl_gd_plateau_reset starts the scheduler over at
        every switch (best = +inf, no bad epochs; lr stays).  graph: every segment replays its own captured graph (no history then); the
        naming and reset launches sit between the replays.  The loss the chain reports — the last history rows, result(), winners() — is
        the last segment's: the plain sampling loss at full resolution.  ValueError: a depth mask, weight_sets, a weighted cloud (or a
        robust plane switched on), pyramids of differing sizes, fewer levels than len(iters).  -> history or None"""
        iters, pyramids = [int(i) for i in iters], list(pyramids)
        if not iters or any(not 0 < i < num_iter for i in iters) or any(b <= a for a, b in zip(iters, iters[1:])):
            raise ValueError("run_pyramid: iters %r: strictly increasing iteration counts inside (0, %d)" % (iters, num_iter))
        if self._chain is not None or self.hyper.depth_mask:
            raise ValueError("run_pyramid: no depth mask (the z-buffer's grid belongs to one panorama size)")
        if self.weight_sets or self._run_weights() is not None:
            raise ValueError("run_pyramid: an engine without weight_sets over a cloud without weights")
        I, L = len(pyramids), len(iters)
        if I < 1 or self.B % I or (self.cloud.color_sets > 1 and I != self.cloud.color_sets):
            raise ValueError("run_pyramid: %d pyramids for %d candidates over %d colour sets" % (I, self.B, self.cloud.color_sets))
        if any(p.levels < L for p in pyramids):
            raise ValueError("run_pyramid: %d switches need pyramids of at least %d coarse levels" % (L, L))
        for l in range(L + 1):
            _same_texels([p.panos[l] for p in pyramids], pyramids[0].panos[l], "run_pyramid: the pyramids must share sizes and texel formats, level by level")
        # one stand-in panorama per size and format for good: it is the launches' default (a captured graph holds its address), every
        # candidate reads the panorama its pose record names
        kept = self.__dict__.setdefault("_level_panos", {})
        hists, done = [], 0
        for s, end in enumerate(iters + [int(num_iter)]):
            level = [p.panos[L - s] for p in pyramids]
            self.pano = kept.setdefault(level[0].texels, level[0])
            self.set_pano_groups(level)
            if s and reset_plateau:
                _checked("pcl_gd_plateau_reset", _ptr(self.state), self.B, _stream())
            if graph:
                self.run_graph(end - done)
            else:
                hists.append(self.run(end - done, history))
            done = end
        return torch.cat(hists) if history and not graph else None

    def reset(self, trans, rot):
        """Re-initialise the optimiser state for new starting poses (same cloud / panorama / B): lets one captured
        graph serve many refinements."""
        if self._chain is not None:
            return self._chain.reset(trans, rot)
        trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
        assert trans.shape[0] == self.B
        if self.weight_sets:
            _checked("pcl_gd_init_weight_sets", _ptr(self.state), _ptr(trans), _ptr(rot), self.B, self.weight_sets, ctypes.byref(self.hyper), _stream())
            return
        _checked("pcl_gd_init", _ptr(self.state), _ptr(trans), _ptr(rot), self.B, ctypes.byref(self.hyper), _stream())

    def set_panos(self, panos):
        """Candidate b samples panos[b] (a list of B Pano objects, all the size / texel format of self.pano): lets the
        candidates of several query images share one launch chain.  Call after __init__ / reset()."""
        assert len(panos) == self.B
        _same_texels(panos, self.pano)
        self._panos = list(panos)                      # keep them alive
        self.set_pano_table(torch.tensor([p.data.data_ptr() for p in panos], dtype=torch.int64, device=self.state.device),
                            images=len({id(p) for p in panos}))

    def set_pano_table(self, table, images=0):
        """Same with a ready-made device tensor of B packed-panorama addresses (int64); the caller keeps the Pano
        objects alive.  No host work besides the launch.  `images`: how many query images the table names (image i's candidates
        a contiguous range) — a hint for the block -> XCD mapping of the launches, results do not depend on it."""
        self.hyper.images = int(images)
        assert table.dtype == torch.int64 and table.numel() == self.B and table.is_cuda
        _checked("pcl_gd_set_panos", _ptr(self.state), _ptr(table), self.B, _stream())
        self._pano_table = table

    def set_pano_groups(self, panos):
        """Candidates [i * B / I, (i + 1) * B / I) sample panos[i] (I Pano objects of the size / texel format of self.pano, B
        divisible by I).  Unlike set_panos / set_pano_table nothing is copied to the device: the addresses are kernel arguments."""
        self._name_panos(panos)
        self.hyper.images = len(panos)                 # (mapping hint for pcl_gd_run: the XCDs split the images)

    def winner(self, nimages=1, leaf_trans=None, leaf_rot=None):
        """(nimages, 16) GPU tensor: per image of B / nimages candidates the one omniloc_batch returns (_GdEngine.winners)."""
        return self.winners(nimages, leaf_trans, leaf_rot)

    def _groups(self):
        """the images whose candidates share this chain: the cloud's colour sets, else what set_pano_groups / set_panos named, else one"""
        return max(1, int(self.cloud.color_sets), int(self.hyper.images))

    def _same_problem(self, other):
        return other.cloud.n == self.cloud.n and other.cloud.color_sets == self.cloud.color_sets and other.pano.texels == self.pano.texels

    def _smaller(self, keep):
        if self.weight_sets:
            raise ValueError("pruned: a weight-set engine is not pruned")
        return super()._smaller(keep)

    def step_from_grads(self, loss, grad):
        """Teacher-forcing hook (tests): ONE optimiser step of every candidate from a GIVEN loss (B,) and gradient (B, 6) =
        dL/d(t0, t1, t2, yaw, pitch, roll) through the epilogue's own Adam / ReduceLROnPlateau / clamp code (pcl_gd_step_from_grads)."""
        loss, grad = _dev(loss).reshape(self.B), _dev(grad).reshape(self.B, 6)
        scratch = torch.empty(self.B * 8, dtype=F32, device=self.state.device)
        _checked("pcl_gd_step_from_grads", _ptr(self.state), self.B, _ptr(loss), _ptr(grad), _ptr(self.box), ctypes.byref(self.hyper), _ptr(scratch), _stream())


class GradientDescentRoomsImages(_GdEngine):
    """On-device GD refinement of SEVERAL panoramas against several rooms in one launch chain (pcl_gd_run_rooms_images): `rooms` is a list
    of (Cloud, box) pairs, `panos` a list of I Pano objects of one size and texel format, `trans` / `rot` hold nrooms * I * per_image rows
    and candidate (r, i, j) is row (r * I + i) * per_image + j.  Every room cloud holds one colour set (the images share the room's colours)
    or I of them (Cloud.with_color_sets: image i reads set i of every room).  The results of every (room, image) equal those of a
    GradientDescent over that room and image alone, bit for bit.  At most PCL_GD_MAX_ROOMS rooms."""

    _INHERITED, _GROUP = ("pano", "clouds", "nrooms", "nimages", "color_sets", "boxes", "depth_mask", "_rooms"), "(room, image)"

    def __init__(self, rooms, panos, trans, rot, lr=0.1, patience=5, factor=0.9, batch_mode=True, fuse=None, depth_mask=False, depth_tau=None,
                 depth_res=None, depth_stride=None, name_panos=True):
        """depth_mask: the scatter-min depth mask in the chain (pcl_gd_run_depth_chain): every room on its own grid, as
        GradientDescent(depth_mask=True) of that room resolves it; depth_res applies to every room.  name_panos False: the pose records name
        no panorama and every candidate samples panos[0], the kernel argument, until set_panos."""
        name = type(self).__name__
        if not 1 <= len(rooms) <= _lib.GD_MAX_ROOMS:
            raise ValueError("%s: %d rooms (1..%d per chain)" % (name, len(rooms), _lib.GD_MAX_ROOMS))
        if len(panos) < 1:
            raise ValueError("%s: no panorama" % name)
        self.pano = panos[0]
        self.clouds = [c for c, _ in rooms]
        for c in self.clouds:
            _unweighted(c, name)
        self.nrooms, self.nimages = len(rooms), len(panos)
        sets = {int(c.color_sets) for c in self.clouds}
        if len(sets) != 1 or sets.pop() not in (1, self.nimages):
            raise ValueError("%s: every room cloud needs one colour set, or one per image (%d)" % (name, self.nimages))
        self.color_sets = int(self.clouds[0].color_sets)
        self.boxes = [_dev(b).reshape(6) for _, b in rooms]
        trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
        B = int(trans.shape[0])
        if B % (self.nrooms * self.nimages) or B == 0:
            raise ValueError("%s: %d candidates do not split into %d rooms x %d images" % (name, B, self.nrooms, self.nimages))
        self.depth_mask = bool(depth_mask)
        self.hyper = _gd_hyper(lr, patience, factor, batch_mode, fuse,
                               _chain_depth_args([c.n for c in self.clouds], self.pano.H, self.pano.W, depth_res, depth_tau, depth_stride)
                               if depth_mask else None, self.color_sets if self.color_sets > 1 else 0)
        self._rooms = (_lib.GdRoom * self.nrooms)(*[_lib.GdRoom(c.data.data_ptr(), c.n, b.data_ptr()) for c, b in zip(self.clouds, self.boxes)])
        self._size(B)
        self._allocate()
        self.reset(trans, rot)
        if name_panos:
            self.set_panos(panos)

    def _size(self, B):
        self.B, self.per_room, self.per_image = B, B // self.nrooms, B // self.nrooms // self.nimages
        self._shape = (self._rooms, self.nrooms, self.nimages, self.per_image)        # (how every pcl_gd_*rooms_images / *depth_chain call begins)

    def _workspace_bytes(self):
        if self.depth_mask:
            return _lib.load().pcl_gd_depth_chain_workspace_bytes(*self._shape, self.pano.H, self.pano.W, ctypes.byref(self.hyper))
        return _lib.load().pcl_gd_rooms_images_workspace_bytes(*self._shape, ctypes.byref(self.hyper))

    def _refusal(self, smaller):
        return "pcl_gd_%s_workspace_bytes: invalid arguments" % ("depth_chain" if self.depth_mask else "rooms_images")

    def plan(self):
        """-> (nchunks per room, poses per block, fused): pcl_gd_plan_rooms_images; with the depth mask (never fused) a fourth item, per room
        (depth_h, depth_w, occluder stride): pcl_gd_plan_depth_chain"""
        arr = lambda: (ctypes.c_int * self.nrooms)()      # noqa: E731
        nch, G = arr(), ctypes.c_int(0)
        if self.depth_mask:
            dh, dw, st = arr(), arr(), arr()
            _checked("pcl_gd_plan_depth_chain", *self._shape, self.pano.H, self.pano.W, ctypes.byref(self.hyper), nch, ctypes.byref(G), dh, dw, st)
            return list(nch), G.value, False, list(zip(dh, dw, st))
        fused = ctypes.c_int(0)
        _checked("pcl_gd_plan_rooms_images", *self._shape, ctypes.byref(self.hyper), nch, ctypes.byref(G), ctypes.byref(fused))
        return list(nch), G.value, bool(fused.value)

    def reset(self, trans, rot):
        """New starting poses for the same rooms / shape, which lets one captured graph serve many refinements (the pose records then name no
        panorama: call set_panos)."""
        trans, rot = _dev(trans).reshape(-1, 3), _dev(rot).reshape(-1, 3)
        assert trans.shape[0] == self.B
        _checked("pcl_gd_init_rooms_images", _ptr(self.state), _ptr(trans), _ptr(rot), self.nrooms, self.nimages, self.per_image,
                 ctypes.byref(self.hyper), _stream())

    def set_panos(self, panos):
        """Image i's candidates in every room sample panos[i] (addresses as kernel arguments: no copy to the device)."""
        if len(panos) != self.nimages:
            raise ValueError("%s: %d panoramas for %d images" % (type(self).__name__, len(panos), self.nimages))
        self._name_panos(list(panos) * self.nrooms)

    def run(self, num_iter, history=False, timer=None):
        hist = torch.empty(num_iter, self.B, dtype=F32, device=self.state.device) if history else None
        _checked("pcl_gd_run_depth_chain" if self.depth_mask else "pcl_gd_run_rooms_images", self._rooms, self.nrooms, self.nimages,
                 _ptr(self.pano.data), self.pano.fmt, self.pano.H, self.pano.W, _ptr(self.state), self.per_image, ctypes.byref(self.hyper), int(num_iter),
                 _ptr(hist), _ptr(self.ws), self.ws_bytes, timer.handle if timer else None, _stream())
        return hist

    def winner(self, leaf_trans=None, leaf_rot=None):
        """(nrooms * nimages, 16): per (room, image), room by room, the candidate omniloc_batch returns (_GdEngine.winners)."""
        return self.winners(self.nrooms * self.nimages, leaf_trans, leaf_rot)

    def _groups(self):
        return self.nrooms * self.nimages

    def _same_problem(self, other):
        return (other.nrooms, other.nimages, other.color_sets, other.depth_mask) == (self.nrooms, self.nimages, self.color_sets, self.depth_mask) and \
            [c.n for c in other.clouds] == [c.n for c in self.clouds] and other.pano.texels == self.pano.texels


class GradientDescentRooms(GradientDescentRoomsImages):
    """On-device GD refinement of ONE panorama against several rooms in one launch chain: the engine's one-image case (the C side forwards
    nimages = 1 to pcl_gd_run_rooms).  `rooms` is a list of (Cloud, box) pairs without colour sets, `trans` / `rot` hold nrooms * per_room
    rows, room r's candidates the rows [r * per_room, (r + 1) * per_room).  Takes the engine's further arguments; the eager chain samples the
    kernel-argument panorama, so the pose records name none until set_panos."""

    def __init__(self, rooms, pano, trans, rot, *args, **kwargs):
        if any(c.color_sets > 1 for c, _ in rooms):
            raise ValueError("GradientDescentRooms: a room cloud with colour sets")
        super().__init__(rooms, [pano], trans, rot, *args, name_panos=False, **kwargs)


class KernelTimer:
    """HIP-event pairs around every fused loss+gradient launch of GradientDescent.run (measurement aid)."""

    def __init__(self, capacity, stride=1):
        self.handle = ctypes.c_void_p(_lib.load().pcl_timer_create(int(capacity)))
        if not self.handle:
            raise _lib.PiccoloHipError("pcl_timer_create failed")
        _lib.load().pcl_timer_set_stride(self.handle, int(stride))

    def reset(self):
        _lib.load().pcl_timer_reset(self.handle)

    def read(self):
        """(total kernel ms, launches) since the last reset; synchronises on the recorded events."""
        ms, cnt = ctypes.c_double(0), ctypes.c_int(0)
        _checked("pcl_timer_read", self.handle, ctypes.byref(ms), ctypes.byref(cnt))
        return ms.value, cnt.value

    def calibrate(self, reps=64):
        """Median reading (ms) of an event pair with NOTHING between its two records, on the current stream: what a pair around
        a kernel over-reads.  Synchronises."""
        ms = ctypes.c_double(0)
        _checked("pcl_timer_calibrate", self.handle, int(reps), ctypes.byref(ms), _stream())
        return ms.value

    def __del__(self):
        try:
            if self.handle:
                _lib.load().pcl_timer_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def cloud2idx(xyz):
    x = _dev(xyz)
    shp = x.shape
    flat = x.reshape(-1, 3)
    out = torch.empty(flat.shape[0], 2, dtype=F32, device=x.device)
    if flat.shape[0]:
        _checked("pcl_cloud2idx", _ptr(flat), int(flat.shape[0]), _ptr(out), _stream())
    return out.reshape(shp[:-1] + (2,))


def sample_from_img(pano, coord):
    c = _dev(coord)
    shp = c.shape
    flat = c.reshape(-1, 2)
    out = torch.empty(flat.shape[0], 3, dtype=F32, device=c.device)
    if flat.shape[0]:
        _checked("pcl_sample_from_img", _ptr(pano.data), pano.fmt, pano.H, pano.W, _ptr(flat), int(flat.shape[0]), _ptr(out), _stream())
    return out.reshape(shp[:-1] + (3,))


def cloud2idx_backward(xyz, grad_coord):
    """grad w.r.t. xyz (.., 3) of cloud2idx for the incoming gradient grad_coord (.., 2)."""
    x, g = _dev(xyz), _dev(grad_coord)
    flat, gflat = x.reshape(-1, 3), g.reshape(-1, 2)
    if gflat.shape[0] != flat.shape[0]:
        raise ValueError("grad_coord must have one (gx, gy) per point")
    out = torch.empty_like(flat)
    if flat.shape[0]:
        _checked("pcl_cloud2idx_backward", _ptr(flat), _ptr(gflat), int(flat.shape[0]), _ptr(out), _stream())
    return out.reshape(x.shape)


def sample_from_img_backward(pano, coord, grad_rgb, want_coord=True, want_img=False):
    """(grad_coord (.., 2) or None, grad_img (H, W, 3) or None) of sample_from_img for the incoming gradient grad_rgb (.., 3)."""
    c, g = _dev(coord), _dev(grad_rgb)
    flat, gflat = c.reshape(-1, 2), g.reshape(-1, 3)
    if gflat.shape[0] != flat.shape[0]:
        raise ValueError("grad_rgb must have one colour per coordinate")
    gc = torch.empty_like(flat) if want_coord else None
    gi = torch.zeros(pano.H, pano.W, 3, dtype=F32, device=c.device) if want_img else None
    if flat.shape[0] and (want_coord or want_img):
        _checked("pcl_sample_from_img_backward", _ptr(pano.data), pano.fmt, pano.H, pano.W, _ptr(flat), _ptr(gflat), int(flat.shape[0]), _ptr(gc), _ptr(gi),
                 _stream())
    elif gc is not None:
        gc.zero_()
    return (gc.reshape(c.shape) if gc is not None else None), gi


def rot_from_ypr(rot):
    r = _dev(rot).reshape(-1, 3)
    out = torch.empty(r.shape[0], 9, dtype=F32, device=r.device)
    _checked("pcl_rot_from_ypr", _ptr(r), int(r.shape[0]), _ptr(out), _stream())
    return out.reshape(-1, 3, 3)


def transform_cloud(xyz, trans, rot):
    x = _dev(xyz)
    t, r = _dev(trans).reshape(3), _dev(rot).reshape(3)
    out = torch.empty_like(x)
    _checked("pcl_transform_cloud", _ptr(x), int(x.shape[0]), _ptr(t), _ptr(r), _ptr(out), _stream())
    return out


def make_pano(xyz_cam, rgb, resolution):
    """(H, W, 3) float GPU tensor = rgb*255 of the winning point per pixel (utils.py:134-205 semantics)."""
    x, c = _dev(xyz_cam), _dev(rgb)
    H, W = int(resolution[0]), int(resolution[1])
    img = torch.empty(H, W, 3, dtype=F32, device=x.device)
    ws = _bytes(H * W * 8)
    _checked("pcl_make_pano", _ptr(x), _ptr(c), int(x.shape[0]), H, W, _ptr(img), _ptr(ws), _stream())
    return img


def scatter_min_depth(xyz_cam, resolution):
    """torch_scatter-style (zmin (H*W,), argmin (H*W,)) of point depth per make_pano pixel; empty -> (0, n)."""
    x = _dev(xyz_cam)
    H, W = int(resolution[0]), int(resolution[1])
    n = int(x.shape[0])
    zbuf = _bytes(H * W * 8)
    zmin = torch.empty(H * W, dtype=F32, device=x.device)
    arg = torch.empty(H * W, dtype=torch.int64, device=x.device)
    _checked("pcl_scatter_min_depth", _ptr(x), n, H, W, _ptr(zbuf), _stream())
    _checked("pcl_scatter_min_unpack", _ptr(zbuf), n, H, W, _ptr(zmin), _ptr(arg), _stream())
    return zmin, arg
