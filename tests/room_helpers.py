"""Scene builders the room-search tests share (tests/test_room_search.py, test_room_images.py, test_enqueue_sequence.py): rooms side by side
in one frame on the GPU, the panorama one of them shows, starting poses per (room, image) and per-image colours of every room."""
import torch


def rooms(sizes, seed=0):
    from piccolo_amd import synth
    return [(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()) for x, c in synth.rooms_side_by_side(sizes, seed)]


def query(rooms, r, seed, res=(256, 512)):
    """the panorama room r shows from room_gt_pose(r, seed) (its own cloud: the walls hide the other rooms)"""
    from piccolo_amd import ops, synth
    t, ypr = synth.room_gt_pose(r, seed)
    xyz, rgb = rooms[r]
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(xyz, torch.from_numpy(t), torch.from_numpy(ypr)), rgb, res))
    return img, t, ypr


def image_starts(nrooms, nimages, per_image, seed=3):
    """starts[r][i] = (trans, rot) of image i in room r: around room r's ground-truth pose, another draw per image"""
    from piccolo_amd import synth
    out = []
    for r in range(nrooms):
        t, ypr = synth.room_gt_pose(r, seed + r)
        row = []
        for i in range(nimages):
            tr, ro = synth.start_poses(t, ypr, per_image, seed=seed + 7 * r + 101 * i, sigma_t=0.4, sigma_r=0.2)
            row.append((torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()))
        out.append(row)
    return out


def per_image_colours(rooms, nimages, seed=0):
    """rooms whose rgb is a list: image i's own colours of every room (a per-image perturbation of the room's rgb, as color_mod gives)"""
    out = []
    for r, (xyz, rgb) in enumerate(rooms):
        g = torch.Generator(device="cpu").manual_seed(seed + 13 * r)
        cols = []
        for i in range(nimages):
            gain = 0.8 + 0.05 * i
            noise = (torch.rand(rgb.shape, generator=g) * 0.1).to(rgb.device)
            cols.append((rgb * gain + noise).clamp(0, 1).contiguous())
        out.append((xyz, cols))
    return out
