"""The depth mask's z-buffers, word for word (csrc/pcl_depth.hip).

A z-buffer is a min-reduction of integer keys, so (1) every z-pass form — LDS window with and without the second window, the window
of grids that are not dense, the coarse-tile cache, the untiled scatter — must leave the same words, and (2) those words are a function
of the occluder samples alone: rule (a)/(b) of tests/depth_helpers.py against a float64 model, with a band for the samples that fp32
may legitimately put into a neighbouring cell (delta, rho: the model's own fp32-vs-fp64 gap x 3, computed per case).  (3) The mark
pass and the loss kernel's lookup read those words; (4) the loss launch's per-block reset of the other z-buffer set covers every word
at extreme ratios of words to blocks.  The rule itself is tested on the CPU: the oracle's scatter-min passes, a lost sample, a planted
word and two swapped cells fail."""
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_helpers as dh
from conftest import REPO

gpu = pytest.mark.gpu

# the six settings of the cross-form comparison: the shipped library, then the experiments library with its A/B knobs
SETTINGS = {
    "shipped": None,
    "exp": {},
    "exp ZFORM=1": {"PCL_ZFORM": "1"},
    "exp ZFORM=2": {"PCL_ZFORM": "2"},
    "exp ZFORM=2 ZSECOND=0": {"PCL_ZFORM": "2", "PCL_ZSECOND": "0"},
    "exp ZFORM=3": {"PCL_ZFORM": "3"},
}


@pytest.fixture(scope="module")
def scene():
    xyz, rgb = dh.occluder_scene()
    assert len(xyz) == 33768 == 8 * 4096 + 1000
    trans, rot = dh.case_poses()
    return xyz, rgb, trans, rot


def _model(scene, case, order):
    xyz, rgb, trans, rot = scene
    k = dh.CASES[case]
    return dh.CaseModel(dh.case_points(case, xyz, rgb)[0][order], trans, rot, k["grid"], k["stride"], k["tau"])


# ===================================================================================================== the rule itself (CPU)
CPU_CASES = ("W1", "W4", "W6", "C1")       # (their grids and strides; the identity order stands in for the device's)


@pytest.fixture(scope="module")
def cpu_models(scene):
    return {c: _model(scene, c, np.arange(len(scene[0]))) for c in CPU_CASES}


@pytest.mark.parametrize("case", CPU_CASES)
def test_rule_accepts_the_fp32_oracle(scene, cpu_models, oracle, case):
    """The oracle's fp32 scatter-min over the same samples (depths squared) is a legitimate z-buffer: rule (a)/(b) holds, and the band
    stays under its cap."""
    xyz, rgb, trans, rot = scene
    cm = cpu_models[case]
    assert 0 < cm.delta < 0.5 and 0 < cm.rho < 1e-4, (cm.delta, cm.rho)
    for b in range(dh.B_POSES):
        cam32 = dh.camera_points(xyz, trans[b], rot[b], np.float32)[cm.samples()]
        zmin, _ = oracle.scatter_min_depth(cam32, (cm.Hd, cm.Wd))
        z = dh.values_to_words(np.where(zmin == 0, np.inf, zmin.astype(np.float64) ** 2))
        res = dh.check_zbuffer(cm, b, z)
        assert res.border_share <= dh.BORDER_CAP, (case, b, res.border_share)
        assert len(res.lost) == 0 and len(res.invented) == 0, (case, b, res.lost[:5], res.invented[:5])
        assert res.pure_cells > 0.5 * (z != dh.Z_INF).sum() and res.worst <= cm.rho, (case, b, res.pure_cells, res.worst, cm.rho)


def _pure_minimum(cm, b):
    """(cell, sample): an interior sample that is the minimum of a cell with several samples, the runner-up well above it"""
    val, cell, border = cm.poses[b].val[cm.samples()], cm.cell(b), cm.border(b)
    ccell, csamp = cm.candidates(b)
    touched = np.zeros(cm.Hd * cm.Wd, bool)
    touched[ccell[border[csamp]]] = True
    o = np.lexsort((val, cell))
    for i in range(len(o) - 1):
        s, t = o[i], o[i + 1]
        if (i == 0 or cell[o[i - 1]] != cell[s]) and cell[t] == cell[s] and not touched[cell[s]] and val[t] > val[s] * (1 + 100 * cm.rho):
            return int(cell[s]), int(s)
    raise AssertionError("no such cell")


@pytest.mark.parametrize("case", CPU_CASES)
def test_rule_rejects_a_lost_sample_a_planted_word_and_swapped_cells(cpu_models, case):
    cm, b = cpu_models[case], 1
    z = dh.reference_zbuffer(cm, b)
    res = dh.check_zbuffer(cm, b, z)
    assert len(res.lost) == 0 and len(res.invented) == 0 and res.worst <= cm.rho
    # (a): the z-buffer recomputed without one interior sample that is its cell's minimum
    cell, s = _pure_minimum(cm, b)
    res = dh.check_zbuffer(cm, b, dh.reference_zbuffer(cm, b, skip=s))
    assert list(res.lost) == [s] and len(res.invented) == 0 and res.worst > cm.rho
    # (b): one word planted in a cell no sample can reach
    reach = np.zeros(z.size, bool)
    reach[cm.candidates(b)[0]] = True
    empty = np.nonzero(~reach)[0]
    assert len(empty) > 0 and (z[empty] == dh.Z_INF).all()
    planted = z.copy()
    planted[empty[len(empty) // 2]] = z[cell]
    res = dh.check_zbuffer(cm, b, planted)
    assert list(res.invented) == [empty[len(empty) // 2]] and len(res.lost) == 0
    # two cells swapped: the smaller word sits in the wrong cell (invented there) and the other cell lost its minimum
    cell2 = next(c for c in np.nonzero(z != dh.Z_INF)[0] if dh.words_to_f64(z[c:c + 1])[0] > dh.words_to_f64(z[cell:cell + 1])[0] * (1 + 100 * cm.rho))
    swapped = z.copy()
    swapped[cell], swapped[cell2] = z[cell2], z[cell]
    res = dh.check_zbuffer(cm, b, swapped)
    assert len(res.lost) > 0 and set(cm.cell(b)[res.lost]) == {cell}
    assert cell2 in set(res.invented)


def test_rule_decides_visibility_of_the_models_own_zbuffer(cpu_models):
    """expected_visible on the model's own z-buffer: what it decides agrees with d2 <= Z in float64, every cell's clear minimum is
    visible although it ties with its own word, and what it leaves out stays under the cap."""
    for case in CPU_CASES:
        cm = cpu_models[case]
        z = dh.reference_zbuffer(cm, 0)
        expect, decided = dh.expected_visible(cm, 0, z)
        assert 1.0 - decided.mean() <= dh.LEFT_OUT_CAP, (case, 1.0 - decided.mean())
        zc = dh.words_to_f64(z)[cm.cell(0, slice(None))]
        tie = np.abs(cm.poses[0].d2 - zc) <= cm.rho * zc
        assert (expect[decided & ~tie] == (cm.poses[0].d2 <= zc)[decided & ~tie]).all()
        assert (decided & tie).sum() > 0.9 * (z != dh.Z_INF).sum() and expect[decided & tie].all(), case


# ===================================================================================================== the device (GPU)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture(scope="module")
def ops():
    _need_gpu()
    from piccolo_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """One child process per setting, each started fresh, one after the other (the knobs are read once per process and exist in the
    experiments build only): every case's z-buffers and byte masks of pcl_depth_mask."""
    _need_gpu()
    from piccolo_amd import build as hip_build
    exp_so = hip_build.build_experiments()                  # (prebuilt by __graft_entry__.build(); compiled here if missing or stale)
    tmp = tmp_path_factory.mktemp("zforms")
    base = {k: v for k, v in os.environ.items() if k not in ("PCL_SO", "PCL_ZFORM", "PCL_ZSECOND")}
    out = {}
    for i, (name, knobs) in enumerate(SETTINGS.items()):
        path = str(tmp / ("setting%d.npz" % i))
        env = dict(base) if knobs is None else dict(base, PCL_SO=exp_so, **knobs)
        code = "import sys; sys.path.insert(0, %r); import depth_helpers; depth_helpers.dump_cases(%r)" % (os.path.join(REPO, "tests"), path)
        run = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (name, run.stderr[-2000:])
        with np.load(path) as f:
            out[name] = {k: f[k] for k in f.files}
    return out


@pytest.fixture(scope="module")
def models(scene, forms):
    """the float64 model of every case in the DEVICE's point order"""
    return {c: _model(scene, c, forms["shipped"][c + "_order"]) for c in dh.CASES}


@gpu
def test_every_zpass_form_leaves_the_same_words(forms, models):
    """z-buffers and byte masks of all eleven cases, bit for bit across the six settings.  (Forcing the window form on a grid narrower
    than a window takes the cache form.)  A difference is described by the model: confined to the cells a border sample can reach it
    is a rounding difference between two instances of the projection, anywhere else a bug of a form."""
    ref, bad = forms["shipped"], []
    for name, got in forms.items():
        for case in dh.CASES:
            assert np.array_equal(got[case + "_order"], ref[case + "_order"]), (name, case)
            for key in ("_z", "_vis"):
                a, b = got[case + key], ref[case + key]
                assert a.shape == b.shape and a.dtype == b.dtype
                if np.array_equal(a, b):
                    continue
                note = "%s %s%s: %d entries differ from the shipped library's" % (name, case, key, int((a != b).sum()))
                if key == "_z":
                    cm = models[case]
                    for p in range(dh.B_POSES):
                        ccell, csamp = cm.candidates(p)
                        reach = np.zeros(a.shape[1], bool)
                        reach[ccell[cm.border(p)[csamp]]] = True
                        note += "; pose %d: %d cells, %d of them out of the border samples' reach" % (p, int((a[p] != b[p]).sum()), int(((a[p] != b[p]) & ~reach).sum()))
                bad.append(note)
    assert not bad, "\n".join(bad)


@gpu
def test_cases_reach_the_paths_they_are_there_for(forms, models):
    """Computed from the float64 model in the device's point order: block partition, anchor sample, window."""
    def blocks(case):
        return [dh.window_blocks(models[case], b) for b in range(dh.B_POSES)]

    def some(case, pred):
        return any(pred(k) for per_pose in blocks(case) for k in per_pose)
    for case in ("W1", "W7"):
        assert dh.zpass_form(33768, 64, 256) == (4096, 48, 128, True) and all(len(p) == 9 for p in blocks(case))
        assert some(case, lambda k: k["certain"] and k["out_lo"] >= 1 and k["out_hi"] <= 700)          # the queue alone
        assert some(case, lambda k: k["certain"] and k["out_lo"] > 900)                               # the queue overflows (NQ = 768)
        assert some(case, lambda k: k["wraps"]) and some(case, lambda k: k["pole"])
        assert all(p[-1]["short"] and not any(k["short"] for k in p[:-1]) for p in blocks(case))      # the short-run anchor
    assert all(sum(1 for k in p if k["certain"] and k["out_lo"] > 900) * 2 >= len(p) for p in blocks("W2")), [[k["out_lo"] for k in p] for p in blocks("W2")]
    assert dh.zpass_form(33768, 128, 256) == (2048, 64, 128, False) and all(len(p) == 17 for p in blocks("W3"))
    assert some("W3", lambda k: k["certain"] and k["out_lo"] >= 1) and some("W3", lambda k: k["wraps"])
    assert dh.zpass_form(16884, 64, 128) == (4096, 48, 128, True) and all(len(p) == 5 and p[-1]["short"] for p in blocks("W4"))
    assert some("W4", lambda k: k["wraps"])
    assert dh.zpass_form(8442, 64, 128) == (2048, 64, 128, False) and dh.zpass_form(11256, 37, 131) == (4096, 48, 128, True)
    assert dh.zpass_form(33768, 24, 40) is None and dh.zpass_form(11256, 37, 100) is None
    assert forms["shipped"]["T1_z"].shape == (3, 4) and forms["shipped"]["T2_vis"].shape == (3, 1)


@gpu
@pytest.mark.parametrize("case", list(dh.CASES))
def test_the_words_are_right(forms, models, parity, case):
    """Rule (a)/(b) for every pose of the shipped library's z-buffers.

    delta's sanity bound: a band of half a cell would leave nothing interior; rho's: the smallest tolerance the product uses is
    tau = 0.02, a value tolerance must stay orders of magnitude below it (1e-4).  Both are properties of the model, not of the kernel."""
    cm, z = models[case], forms["shipped"][case + "_z"]
    assert z.shape == (dh.B_POSES, cm.Hd * cm.Wd)
    res = [dh.check_zbuffer(cm, b, z[b]) for b in range(dh.B_POSES)]
    tag = "%s %dx%d stride %d tau %g: " % (case, cm.Wd, cm.Hd, cm.stride, cm.tau)
    parity(tag + "delta (cells) = 3 x the model's fp32-vs-fp64 gap", cm.delta, 0.5, cm.gap_cell)
    parity(tag + "rho (relative) = 3 x the model's fp32-vs-fp64 gap", cm.rho, 1e-4, cm.gap_val)
    parity(tag + "border share of the samples (worst pose)", max(r.border_share for r in res), dh.BORDER_CAP)
    for b, r in enumerate(res):
        assert len(r.lost) == 0, "%spose %d: rule (a): %d interior samples lost, first %s" % (tag, b, len(r.lost), r.lost[:8])
        assert len(r.invented) == 0, "%spose %d: rule (b): %d words no candidate explains, first cells %s" % (tag, b, len(r.invented), r.invented[:8])
    parity(tag + "worst relative error of a word (cells with interior candidates only, %d)" % sum(r.pure_cells for r in res), max(r.worst for r in res),
           cm.rho, cm.gap_val)
    assert sum(r.pure_cells for r in res) > 0 or cm.n <= 5


@gpu
@pytest.mark.parametrize("case", ["W1", "W4", "C1", "W7"])
def test_mark_pass_and_lookup_read_those_words(ops, oracle, scene, forms, models, parity, case):
    """With the device's z-buffer Z: every point the model can decide (dh.expected_visible) has visible = (d2 <= Z[cell]) exactly, and
    the loss kernel's own lookup counts the visible points that sample a non-black colour (the byte mask fed to the loss kernel), under
    the tolerance of test_depth_mask_vs_oracle_and_in_the_gd_loop for fused versus byte mask."""
    import torch
    from piccolo_amd import synth
    from parity_helpers import T
    xyz, rgb, trans, rot = scene
    k, cm = dh.CASES[case], models[case]
    cloud, order = dh.make_cloud(ops, case, xyz, rgb)
    assert np.array_equal(order, forms["shipped"][case + "_order"])
    z, vis = dh.run_depth_mask(ops, cloud, trans, rot, k["grid"], k["tau"], k["stride"])
    assert np.array_equal(z, forms["shipped"][case + "_z"]) and np.array_equal(vis, forms["shipped"][case + "_vis"])
    assert set(np.unique(vis)) <= {0, 1}
    left_out = 0.0
    for b in range(dh.B_POSES):
        expect, decided = dh.expected_visible(cm, b, z[b])
        left_out = max(left_out, 1.0 - float(decided.mean()))
        wrong = np.nonzero(decided & (vis[b].astype(bool) != expect))[0]
        assert len(wrong) == 0, "%s pose %d: %d decided points with the wrong visibility, first packed slots %s" % (case, b, len(wrong), wrong[:8])
        assert expect[decided].any() and not expect[decided].all()              # the z-buffer hides something, and not everything
    parity("%s: points left out of the mark check (border + threshold ties, worst pose)" % case, left_out, dh.LEFT_OUT_CAP)
    H, W = 128, 256
    t_gt, ypr_gt = synth.gt_pose(17)
    img = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb, (H, W)).astype(np.float32) / 255
    pano = ops.Pano(T(img))
    via_bytes = ops.sampling_loss(cloud, pano, T(trans), T(rot), visible=torch.from_numpy(vis).cuda()).cpu().numpy()
    fused = ops.sampling_loss(cloud, pano, T(trans), T(rot), depth={"depth_res": k["grid"], "depth_tau": k["tau"], "depth_stride": k["stride"]}).cpu().numpy()
    assert (via_bytes[:, 1] > 0).all() and (via_bytes[:, 1] <= vis.sum(1)).all()
    assert np.abs(fused[:, 1] - via_bytes[:, 1]).max() <= 2, (fused[:, 1], via_bytes[:, 1])


@gpu
@pytest.mark.parametrize("n,B,grid", [(820, 2, (128, 256)), (40001, 16, (2, 2)), (820, 3, (37, 131))],
                         ids=["few blocks, large set", "many blocks, tiny set", "total the block count does not divide"])
def test_the_reset_of_the_other_set_covers_every_word(ops, n, B, grid):
    """A call fills z-buffer set 0 itself; iterations 1.. read what the previous loss launch reset, a slice per block.  run(6) equals
    six run(1) on the same engine bit for bit, on workspaces full of garbage, at extreme ratios of words to blocks: 1,025 points, B = 2,
    128 x 256 (16,384 16-byte words); 50,001 points, B = 16, 2 x 2 (16 words: most blocks have nothing to reset); 1,025 points, B = 3,
    37 x 131.  lr = 0.1: the poses move between iterations, so a stale word is not masked by an identical new one."""
    import torch
    from piccolo_amd import synth
    from parity_helpers import T
    xyz, rgb = dh.occluder_scene(n)
    assert len(xyz) in (1025, 50001)
    H, W = 64, 128
    t_gt, ypr_gt = synth.gt_pose(17)
    trans, rot = synth.start_poses(t_gt, ypr_gt, B, seed=17, sigma_t=0.1, sigma_r=0.05)
    X, C = T(xyz), T(rgb)
    cloud = ops.Cloud(X, C)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, T(t_gt), T(ypr_gt)), C, (H, W)))
    pano, box = ops.Pano(img), ops.quantile_box(X, 0.05)

    def make():
        gd = ops.GradientDescent(cloud, pano, T(trans), T(rot), box, lr=0.1, patience=5, factor=0.8, batch_mode=True, depth_mask=True,
                                 depth_res=grid, depth_tau=ops.depth_tau_rule(grid[0]), depth_stride=1)
        gd.ws = torch.full_like(gd.ws, 0x5A)
        return gd
    whole = make()
    hist = whole.run(6, history=True).cpu().numpy()
    pieces = make()
    steps = np.concatenate([pieces.run(1, history=True).cpu().numpy() for _ in range(6)])
    assert hist.shape == steps.shape == (6, B)
    assert np.array_equal(hist.view(np.uint32), steps.view(np.uint32)), (hist, steps)
    assert np.array_equal(whole.result().cpu().numpy().view(np.uint32), pieces.result().cpu().numpy().view(np.uint32))
    assert np.isfinite(hist).all() and not np.array_equal(hist[0], hist[5])
