"""GPU test of the histogram stage's allocation ladders in ops.py: halve the batch / the group, fall back to the z-buffer splat's small
workspace or to the per-image path.  No allocation failure is provoked: ops._bytes is patched to raise torch.cuda.OutOfMemoryError above a
byte threshold chosen from the library's size queries, every request is recorded, and each restricted result must equal the unrestricted
call bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W, NSH, NSW, K, I = 20_000, 128, 256, 4, 4, 10, 3


@pytest.fixture(scope="module")
def room():
    from piccolo_amd import ops, synth
    xyz, rgb = synth.box_room(N, 11)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    imgs, trs, ros = [], [], []
    for i in range(I):
        t_gt, ypr_gt = synth.gt_pose(110 + i)
        cam = ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr_gt))
        imgs.append(synth.quantise_like_image_file(ops.make_pano(cam, C, (H, W))))
        tr, ro = synth.start_poses(t_gt, ypr_gt, K, seed=120 + i)
        trs.append(torch.from_numpy(tr).cuda())
        ros.append(torch.from_numpy(ro).cuda())
    cloud = ops.Cloud(X, C)
    sets = ops.Cloud.with_color_sets(X, [C, C.flip(1).contiguous(), (0.5 * C).contiguous()], order=cloud.order)
    return cloud, sets, imgs, torch.stack(trs), torch.stack(ros)


@pytest.fixture
def limit(monkeypatch):
    """limit(T): from now on ops._bytes refuses more than T bytes; -> the list of (bytes asked, granted) it fills"""
    from piccolo_amd import ops
    real = ops._bytes

    def set_limit(threshold):
        asked = []

        def _bytes(nbytes):
            asked.append((int(nbytes), nbytes <= threshold))
            if nbytes > threshold:
                raise torch.cuda.OutOfMemoryError("test: no more than %d bytes" % threshold)
            return real(nbytes)

        monkeypatch.setattr(ops, "_bytes", _bytes)
        return asked

    return set_limit


def _sizes():
    from piccolo_amd import _lib
    lib = _lib.load()
    binned = lambda b: lib.pcl_hist_trim_workspace_bytes_n(N, b, H, W, NSH, NSW)                  # noqa: E731  one image, b candidates
    splat = lambda b: lib.pcl_hist_trim_workspace_bytes(b, H, W, NSH, NSW)                        # noqa: E731
    images = lambda m: lib.pcl_hist_trim_images_workspace_bytes(N, m, K, H, W, NSH, NSW)          # noqa: E731  m images of K candidates
    sets = lambda n: lib.pcl_hist_trim_images_sets_workspace_bytes(n, I, I, K, H, W, NSH, NSW)    # noqa: E731
    return binned, splat, images, sets


def test_one_image_halves_its_batch_then_takes_the_splat_workspace(room, limit):
    from piccolo_amd import ops
    cloud, _, imgs, trans, rot = room
    binned, splat, _, _ = _sizes()
    assert splat(1) < binned(1) < binned(2) < binned(3) < binned(5) < binned(10)
    want = ops.hist_trim_scores(imgs[0], cloud, trans[0], rot[0], NSH, NSW, return_parts=True)
    asked = limit(binned(5))                                                # 10 candidates do not fit, 5 do
    got = ops.hist_trim_scores(imgs[0], cloud, trans[0], rot[0], NSH, NSW, return_parts=True)
    assert asked == [(binned(10), False), (binned(5), True)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    asked = limit(splat(1))                                                 # not even one candidate's lists fit: the z-buffer splat, one at a time
    got = ops.hist_trim_scores(imgs[0], cloud, trans[0], rot[0], NSH, NSW, return_parts=True)
    assert asked == [(binned(b), False) for b in (10, 5, 3, 2, 1)] + [(splat(1), True)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_images_halve_their_group_then_take_the_per_image_path(room, limit):
    from piccolo_amd import ops
    cloud, _, imgs, trans, rot = room
    binned, _, images, _ = _sizes()
    assert binned(5) < images(1) < images(2) < images(3)
    want = ops.hist_trim_scores_images(imgs, cloud, trans, rot, NSH, NSW)
    asked = limit(images(2))                                                # three images do not fit, two do: groups of 2 and 1
    got = ops.hist_trim_scores_images(imgs, cloud, trans, rot, NSH, NSW)
    assert asked == [(images(3), False), (images(2), True), (images(1), True)]
    assert torch.equal(got, want)
    asked = limit(binned(5))                                                # not one image's 10 candidates: per image, in batches of 5
    got = ops.hist_trim_scores_images(imgs, cloud, trans, rot, NSH, NSW)
    assert images(1) == binned(10)
    assert asked == [(images(3), False), (images(2), False), (images(1), False), (binned(10), False), (binned(5), True)] + \
        2 * [(images(1), False), (binned(10), False), (binned(5), True)]
    assert torch.equal(got, want)


def test_color_sets_take_the_splat_workspace(room, limit):
    from piccolo_amd import ops
    _, cloud, imgs, trans, rot = room
    _, _, _, sets = _sizes()
    assert sets(0) < sets(N)
    want = ops.hist_trim_scores_images(imgs, cloud, trans, rot, NSH, NSW)
    asked = limit(sets(0))
    got = ops.hist_trim_scores_images(imgs, cloud, trans, rot, NSH, NSW)
    assert asked == [(sets(N), False), (sets(0), True)]
    assert torch.equal(got, want)
