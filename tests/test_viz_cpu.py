"""CPU: the restatements of tests/viz_ref.py against each other, ppt_amd.viz's camera on CPU tensors, the host-side argument
checks of the render and predict entry points, the PNG writer, the palette and the command line of `python -m ppt_amd.viz`."""
import ctypes

import numpy as np
import pytest
import torch

import viz_ref as R


@pytest.mark.parametrize("name", list(R.RENDER_CASES))
def test_sequential_and_vectorised_restatements_agree(name):
    """the loop with a strict `<` depth test and the maximum over 64-bit keys: identical pictures and winner maps"""
    c = R.render_case(name)
    for bg in R.BACKGROUNDS:
        pic, win = R.render_sequential(c["ixyz"], c["colors"], c["H"], c["W"], c["r"], bg)
        assert np.array_equal(win, c["win"])
        assert np.array_equal(pic, c["pictures"][bg])
    share = (c["win"] < 0).mean()
    print(f"VIZ {name}: background share {share:.3f}")
    if name in ("small", "wide_ball"):
        assert 0.10 < share < 0.90                         # neither blank nor fully covered
    if name == "empty":
        assert share == 1.0
    if c["ixyz"].shape[0] >= 8:                            # the tie rule is exercised: an exact duplicate never wins a pixel
        n = c["ixyz"].shape[0]
        assert not np.isin(c["win"], np.arange(n - n // 8, n)).any()


def test_camera_on_cpu_tensors_equals_the_numpy_camera():
    """every coordinate equal, except where the float64 value lies within 1e-9 of an integer (there either neighbour passes);
    the restatement alone has no coordinate in that band for these inputs"""
    from ppt_amd import viz
    xyz = np.random.RandomState(11).rand(4, 257, 3) * 2 - 1
    views = [(0.0, 0.0), (0.3, -0.7), (-1.1, 2.0)]
    want, values = R.camera(xyz, views, 96)
    band = R.in_band(values)
    assert band.sum() == 0, int(band.sum())
    got = viz.camera(torch.from_numpy(xyz), views, 96)
    assert got.dtype == torch.int32 and got.shape == (4, 3, 257, 3) and not got.is_cuda
    got = got.numpy()
    differ = got != want
    assert not (differ & ~band).any()
    assert (np.abs(got - want)[differ] <= 1).all()
    # zoom, float32 input, and the mouse fractions of the reference's window
    want, values = R.camera(xyz.astype(np.float32), viz.views_from_mouse([(0.5, 0.5), (0.2, 0.9)]), 64, zoom=1.1)
    got = viz.camera(torch.from_numpy(xyz.astype(np.float32)), viz.views_from_mouse([(0.5, 0.5), (0.2, 0.9)]), 64, zoom=1.1).numpy()
    assert not ((got != want) & ~R.in_band(values)).any()
    assert viz.views_from_mouse([(0.5, 0.5)]) == [(0.0, 0.0)]
    xa, ya = viz.views_from_mouse([(0.25, 0.75)])[0]
    assert xa == (0.75 - 0.5) * np.pi * 1.2 and ya == (0.25 - 0.5) * np.pi * 1.2


def test_render_and_predict_argument_validation_without_gpu():
    """NULL pointers and non-positive sizes return PPT_EINVAL before any launch; the limits give a zero workspace"""
    from ppt_amd import _lib, ops
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 255) & ~255               # a non-NULL, aligned address that is never dereferenced
    bg = bytes([255, 255, 255])
    assert L.ppt_partseg_predict(None, None, 1, 1, 50, None, None, None, None) == -1
    assert L.ppt_partseg_predict(p, p, 0, 8, 50, p, p, p, None) == -1          # B = 0
    assert L.ppt_partseg_predict(p, p, 2, 0, 50, p, p, p, None) == -1          # N = 0
    assert L.ppt_partseg_predict(p, p, 2, 8, 0, p, p, p, None) == -1           # P = 0
    assert L.ppt_partseg_predict(p, p, 2, 8, 65, p, p, p, None) == -3          # P > 64
    #                      ixyz colors pattern background radius G K n  H   W   out ws  bytes stream
    assert L.ppt_render_balls(None, None, None, None, 4, 1, 1, 1, 8, 8, None, None, 0, None) == -1
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, 4, 8, 8, None, p, 256, None) == -1          # out NULL
    assert L.ppt_render_balls(None, p, p, bg, 4, 1, 1, 4, 8, 8, p, p, 256, None) == -1          # ixyz NULL with n > 0
    assert L.ppt_render_balls(p, p, p, None, 4, 1, 1, 4, 8, 8, p, p, 256, None) == -1           # background NULL
    assert L.ppt_render_balls(p, p, p, bg, 4, 0, 1, 4, 8, 8, p, p, 256, None) == -1             # G = 0
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 0, 4, 8, 8, p, p, 256, None) == -1             # K = 0
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, -1, 8, 8, p, p, 256, None) == -1            # n < 0
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, 4, 0, 8, p, p, 256, None) == -1             # H = 0
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, 4, 8, -3, p, p, 256, None) == -1            # W < 0
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, 4, 8, 8, p, p, 0, None) == -1               # workspace too small
    assert L.ppt_render_balls(p, p, p, bg, 17, 1, 1, 4, 8, 8, p, p, 256, None) == -3            # radius > 16
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, 4, 4097, 8, p, p, 256, None) == -3          # H > 4096
    assert L.ppt_render_balls(p, p, p, bg, 4, 1, 1, 65537, 8, 8, p, p, 256, None) == -3         # n > 65536
    assert L.ppt_render_balls_workspace_bytes(3, 100, 64, 64, 17) == 0
    assert L.ppt_render_balls_workspace_bytes(3, 100, 4097, 64, 4) == 0
    assert L.ppt_render_balls_workspace_bytes(3, 100, 64, 4097, 4) == 0
    assert L.ppt_render_balls_workspace_bytes(3, 65537, 64, 64, 4) == 0
    assert L.ppt_render_balls_workspace_bytes(0, 100, 64, 64, 4) == 0
    assert L.ppt_render_balls_workspace_bytes(3, 100, 64, 64, 16) == 256
    assert L.ppt_render_balls_workspace_bytes(96, 2048, 800, 800, 13) == 768
    assert L.ppt_render_balls_workspace_bytes(1, 0, 4096, 4096, -2) == 256                     # n = 0 and r = max(radius, 1) are fine
    assert ops.render_balls_workspace_bytes(96, 2048, 800, 800, 13) == 768


def test_render_and_predict_have_no_cpu_path():
    from ppt_amd import ops, viz
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.render_balls(torch.zeros(1, 4, 3, dtype=torch.int32), torch.zeros(1, 1, 4, 3), 8, 8, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.partseg_predict(torch.zeros(1, 4, 50), torch.zeros(1, dtype=torch.int64), torch.zeros(50, dtype=torch.int32),
                            torch.zeros(50, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        viz.predict_parts(torch.zeros(1, 4, 50), torch.zeros(1, 4, dtype=torch.int64), R.CATEGORY2PART)


def test_ball_pattern_is_the_restatements():
    """the table the wrapper hands to the kernel: (2 r - 1)^2 rows of (dz, s), dz < 0 outside the circle"""
    from ppt_amd import ops
    for radius in (-3, 1, 2, 5, 13, 16):
        r, pat = R.pattern(radius)
        table = ops.ball_pattern_host(radius)
        side = 2 * r - 1
        assert table.shape == (side * side, 2) and table.dtype == np.float64
        inside = {(dx, dy): (dz, s) for dx, dy, dz, s in pat}
        assert all(abs(dx) < r and abs(dy) < r for dx, dy in inside)
        for dx in range(-(r - 1), r):
            for dy in range(-(r - 1), r):
                row = table[(dx + r - 1) * side + dy + r - 1]
                if (dx, dy) in inside:
                    assert tuple(row) == inside[(dx, dy)] and row[0] > 0
                else:
                    assert row[0] < 0


def test_save_png_round_trips(tmp_path):
    from PIL import Image
    from ppt_amd import viz
    img = np.random.RandomState(2).randint(0, 256, (37, 52, 3)).astype(np.uint8)
    path = viz.save_png(str(tmp_path / "a.png"), torch.from_numpy(img))
    with Image.open(path) as f:
        assert f.mode == "RGB" and np.array_equal(np.asarray(f), img)
    viz.save_png(str(tmp_path / "b.png"), img)
    with Image.open(str(tmp_path / "b.png")) as f:
        assert np.array_equal(np.asarray(f), img)
    with pytest.raises(ValueError):
        viz.save_png(str(tmp_path / "c.png"), img.astype(np.float32))


def test_palette_and_part_colours():
    from ppt_amd import ops, viz
    pal = viz.palette_tensor()
    assert pal.dtype == torch.float32 and pal.shape[0] >= max(8, ops.PARTSEG_MAX_PARTS) and pal.shape[1] == 3
    assert len({tuple(row) for row in pal.tolist()}) == pal.shape[0]           # distinct
    assert pal.min() >= 0 and pal.max() <= 255
    with pytest.raises(ValueError):
        viz.palette_tensor([(1, 2, 3)] * 3)
    labels = torch.tensor([[30, 35, 31], [4, 5, -1]])
    col = viz.part_colors(labels, torch.tensor([30, 4]), pal)
    assert torch.equal(col[0], pal[[0, 5, 1]]) and torch.equal(col[1], pal[[0, 1, 0]])


def test_command_line_accepts_the_flags_of_show_partseg():
    from ppt_amd import viz
    a = viz.parser().parse_args(["--class_choice", "Chair", "--ballradius", "13", "--proj_name", "ulip2_partseg", "--exp_name", "e1",
                                 "--output_dir", "outputs", "--ulip2", "--num_learnable_prompt_tokens", "32",
                                 "--class_name_position", "middle", "--npoints", "2048", "--batch_size", "32", "--gpu", "0",
                                 "--data", "set.npz", "--parts", "parts.json", "--views", "0.5,0.5;0.3,0.7", "--size", "640",
                                 "--out", "pictures"])
    assert a.class_choice == "Chair" and a.ballradius == 13 and a.ulip2 and a.npoints == 2048 and a.size == 640
    assert a.ckpt is None and a.parts == "parts.json" and a.out == "pictures"
    assert len(viz._parse_views(a.views)) == 2 and viz._parse_views(a.views)[0] == (0.0, 0.0)
    a = viz.parser().parse_args(["--class_choice", "Mug", "--ckpt", "checkpoint_best.pt", "--data", "set.npz", "--out", "o"])
    assert a.ckpt == "checkpoint_best.pt" and a.ballradius == 13 and a.batch_size == 32 and not a.ulip2
    assert len(viz._parse_views(a.views)) == len(viz.DEFAULT_VIEWS_MOUSE)
