"""``synthetic.make_scene_batch`` with the stereo partner "s" (what scripts/bench_stereo.py trains on): the image of "s" is frame 0
seen from ``stereo_T`` through the scene's depth field, as frames -1 / +1 are seen from ``("T_gt", f)``.  Checked the way the loss
looks at it: warp each source frame into frame 0 with the ground-truth depth and its pose (the oracle's layers, on the CPU)."""
import torch
import torch.nn.functional as F

from oracle import layers as OL

B, H, W, SEED = 2, 64, 96, 5


def _warp_error(inp, depth, src, T):
    pts = OL.backproject_depth(depth, inp[("inv_K", 0)])
    grid = OL.project_3d(pts, inp[("K", 0)], T, H, W)
    warped = F.grid_sample(src, grid, padding_mode="border", align_corners=False)
    inside = (grid.abs().amax(-1) < 0.98).unsqueeze(1).float()           # pixels that frame sees
    assert float(inside.mean()) > 0.8
    return float(((warped - inp[("color", 0, 0)]).abs() * inside).sum() / (3 * inside.sum()))


def test_stereo_partner_is_rendered_from_its_pose():
    from fusiondepth_amd import synthetic
    inp = synthetic.make_scene_batch(B, H, W, frame_ids=[0, -1, 1, "s"], seed=SEED, device="cpu", scatter=lambda b: torch.cat([b, b], 1))
    gen = torch.Generator(device="cpu")
    gen.manual_seed(SEED)
    depth = synthetic.scene_depth(B, H, W, gen, "cpu") / 26.0             # the batch's first draw: its ground-truth depth, in units
    T = inp["stereo_T"]
    eye = torch.eye(4).repeat(B, 1, 1)
    assert T.shape == (B, 4, 4) and torch.equal(T[:, :3, :3], eye[:, :3, :3])
    assert torch.equal(T[:, 1:, 3], eye[:, 1:, 3]) and bool((T[:, 0, 3] < 0).all())      # an "l" item, not flipped: -baseline
    assert ("T_gt", "s") not in inp and ("2channel", "s", 0) not in inp
    temporal = max(_warp_error(inp, depth, inp[("color", f, 0)], inp[("T_gt", f)]) for f in (-1, 1))
    stereo = _warp_error(inp, depth, inp[("color", "s", 0)], T)
    ident = _warp_error(inp, depth, inp[("color", "s", 0)], eye)
    mirrored = _warp_error(inp, depth, inp[("color", "s", 0)], 2 * eye - T)
    print("warp error: temporal frames %.4f, stereo partner %.4f (identity pose %.4f, baseline of the other sign %.4f)"
          % (temporal, stereo, ident, mirrored))
    # Every rendered frame carries the same two resamplings and the same 1 % image noise, so "s" warps back as well as the temporal
    # frames do (25 % margin for the different sub-pixel phases); a partner that is not the scene seen from stereo_T is as far off
    # as a wrong pose is: several times that.
    assert stereo <= 1.25 * temporal
    assert ident >= 3 * stereo and mirrored >= 3 * stereo
    for s in range(1, 4):
        assert torch.equal(inp[("color", "s", s)], F.avg_pool2d(inp[("color", "s", 0)], 2 ** s))


def test_scene_batch_without_stereo_is_unchanged_by_the_stereo_branch():
    from fusiondepth_amd import synthetic
    scat = lambda b: torch.cat([b, b], 1)
    a = synthetic.make_scene_batch(B, H, W, seed=SEED, device="cpu", scatter=scat)
    b = synthetic.make_scene_batch(B, H, W, frame_ids=[0, -1, 1, "s"], seed=SEED, device="cpu", scatter=scat)
    for f in (0, -1, 1):
        assert torch.equal(a[("color", f, 0)], b[("color", f, 0)])
    assert "stereo_T" not in a
