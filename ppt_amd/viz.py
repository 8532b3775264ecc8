"""Part-segmentation pictures on the device: the counterpart of notebook/show_balls.py (+ show-partseg.sh), headless.

The reference loads checkpoint_best.pt, runs the part-seg model on a batch, takes the category-masked arg-max per point
(show_balls.py:256-262) and draws ONE cloud in an OpenCV window through a prebuilt render_ball binary.  Here the per-point
predictions are a public call and the drawing is a kernel (csrc/render.hip): contact sheets of ground truth, prediction and their
disagreement over several views, for a whole batch in one launch, written as PNG.

    pred = predict_parts(logits, part_label, category2part)                      # [B, N] int32, show_balls.py:256-262
    ixyz = camera(pc, views_from_mouse([(0.5, 0.5), (0.3, 0.7)]), size=800)      # [B, V, N, 3] int32, show_balls.py:73-75, 97-119
    img = render_balls(ixyz, colors, 800, radius=13)                             # [B, V, K, 800, 800, 3] uint8
    sheets = partseg_sheet(model, pc, cls_label, part_label, category2part)      # [B, rows * 800, views * 800, 3] uint8
    save_png("chair_0.png", sheets[0])
    python -m ppt_amd.viz --class_choice Chair --ckpt checkpoint_best.pt --data test.npz --out pictures/

The pictures are this project's own statement of the ball splat (include/ppt_hip.h: ppt_render_balls); parity with the
reference's binary is not claimed.  Its window, mouse and key handling, `magnifyBlue`, the text overlay, the BGR channel order and
its colour table (which gives parts 3-9 one colour) are not reproduced: channels are RGB, every part has its own colour.
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import evaluate, ops

DEFAULT_VIEWS_MOUSE = ((0.5, 0.5), (0.35, 0.65), (0.7, 0.25))      # the reference's mouse fractions (x, y); (0.5, 0.5): no rotation

# One colour per part slot of a category (RGB, 0-255): distinct hues at similar lightness, so that the shading stays readable.
PALETTE = ((228, 26, 28), (55, 126, 184), (77, 175, 74), (255, 127, 0), (152, 78, 163), (0, 191, 196), (166, 86, 40), (247, 129, 191),
           (230, 200, 30), (110, 110, 110))
AGREE, DISAGREE = (190, 190, 190), (220, 20, 20)                   # the error map: agreeing points grey, disagreeing red


def views_from_mouse(fractions):
    """[(mousex, mousey)] in [0, 1] -> [(xangle, yangle)] in radians, as show_balls.py:99, :108: angle = (m - 0.5) * 1.2 pi, the
    x-angle from the mouse's y and the y-angle from its x."""
    return [((my - 0.5) * math.pi * 1.2, (mx - 0.5) * math.pi * 1.2) for mx, my in fractions]


def rotation(xangle, yangle, zoom=1.0):
    """show_balls.py:97-116: eye . Rx(xangle) . Ry(yangle) * zoom, a [3, 3] float64 numpy matrix applied as xyz . rotmat"""
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(xangle), -np.sin(xangle)], [0.0, np.sin(xangle), np.cos(xangle)]])
    ry = np.array([[np.cos(yangle), 0.0, -np.sin(yangle)], [0.0, 1.0, 0.0], [np.sin(yangle), 0.0, np.cos(yangle)]])
    return np.eye(3).dot(rx).dot(ry) * zoom


def camera(xyz, views, size, zoom=1.0):
    """xyz [B, N, 3] (any float dtype, any device), views [(xangle, yangle)] in radians -> ixyz [B, V, N, 3] int32 on the same
    device: row, column, depth in pixels of a size x size picture.  show_balls.py:73-75 and :97-119 in float64: centre on the
    mean, divide by (2.2 max norm) / size, rotate by the x-angle then the y-angle, times zoom, add (size / 2, size / 2, 0),
    truncate toward zero.  The 3 x 3 product is written out (no BLAS call), so CPU and device take the same steps."""
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"camera: xyz must be [B, N, 3], got {tuple(xyz.shape)}")
    p = xyz.detach().double()
    p = p - p.mean(dim=1, keepdim=True)
    radius = (p ** 2).sum(dim=-1).sqrt().amax(dim=1)
    p = p / ((radius * 2.2) / float(size)).view(-1, 1, 1)
    rot = torch.from_numpy(np.stack([rotation(xa, ya, zoom) for xa, ya in views])).to(p.device)          # [V, 3, 3]
    x, y, z = (p[:, None, :, k, None] for k in range(3))                                                # [B, 1, N, 1] each
    r = rot[None, :, None, :, :]                                                                        # [1, V, 1, 3, 3]
    out = x * r[..., 0, :] + y * r[..., 1, :] + z * r[..., 2, :]
    out = out + torch.tensor([size / 2, size / 2, 0.0], dtype=torch.float64, device=p.device)
    return out.to(torch.int32)                               # (float -> int conversion truncates toward zero, as astype('int32'))


def _tables(category2part, device):
    start, count = evaluate.part_tables(category2part)
    return torch.from_numpy(start).to(device), torch.from_numpy(count).to(device)


def predict_parts(logits, labels_or_anchor, category2part):
    """logits [B, N, P] on the device; labels_or_anchor: the part labels [B, N] (the cloud's category is that of point 0's label,
    show_balls.py:259) or one part id per cloud [B] -> pred [B, N] int32: the arg-max over the category's parts, plus the
    category's first part (show_balls.py:262); -1 for a cloud whose anchor is no part id.  ops.partseg_predict."""
    anchor = labels_or_anchor[:, 0] if labels_or_anchor.dim() == 2 else labels_or_anchor
    lg, anchor = evaluate._as_inputs(logits, anchor.to(logits.device))
    start, count = _tables(category2part, lg.device)
    return ops.partseg_predict(lg, anchor, start, count)


def render_balls(ixyz, colors, size, radius=10, background=(255, 255, 255)):
    """ixyz [..., n, 3] int32 (row, column, depth: camera()), colors [..., K, n, 3] or [..., n, 3] in [0, 255], on the device ->
    uint8 pictures [..., K, H, W, 3] (RGB; without a K axis in `colors`: [..., H, W, 3]).  size: one number or (H, W).  Every
    point is a shaded ball, the nearest wins; the visibility of a geometry is resolved once for its K colourings
    (ops.render_balls)."""
    H, W = (size, size) if isinstance(size, int) else size
    lead = ixyz.shape[:-2]
    n = ixyz.shape[-2]
    has_k = colors.dim() == ixyz.dim() + 1
    if tuple(colors.shape[:len(lead)]) != tuple(lead) or colors.shape[-2:] != (n, 3) or colors.dim() not in (ixyz.dim(), ixyz.dim() + 1):
        raise ValueError(f"render_balls: colors {tuple(colors.shape)} do not belong to ixyz {tuple(ixyz.shape)}")
    K = colors.shape[-3] if has_k else 1
    G = int(np.prod(lead)) if lead else 1
    out = ops.render_balls(ixyz.reshape(G, n, 3).contiguous(), colors.float().reshape(G, K, n, 3).contiguous(), H, W, radius, background)
    return out.view(*lead, K, H, W, 3) if has_k else out.view(*lead, H, W, 3)


def palette_tensor(palette=None, device="cpu"):
    """-> [>= PPT_PARTSEG_MAX_PARTS, 3] f32 colours in [0, 255]"""
    pal = torch.as_tensor(PALETTE if palette is None else palette, dtype=torch.float32).reshape(-1, 3)
    if pal.shape[0] < ops.PARTSEG_MAX_PARTS:
        raise ValueError(f"palette: {pal.shape[0]} colours for up to {ops.PARTSEG_MAX_PARTS} parts per category")
    return pal.to(device)


def part_colors(labels, start, palette):
    """labels [B, N] (part ids), start [B] (the category's first part) -> [B, N, 3] f32: palette[label - start], clamped into the
    palette (a label outside the category, or -1, takes an end colour instead of faulting)"""
    slot = (labels.long() - start.long().view(-1, 1)).clamp_(0, palette.shape[0] - 1)
    return palette[slot]


def partseg_sheet(model, pc, cls_label, part_label, category2part, views=None, size=800, radius=13, palette=None,
                  error_map=True, background=(255, 255, 255)):
    """One contact sheet per cloud of a batch: columns are the views, rows are ground truth, prediction and (error_map) their
    disagreement -- agreeing points grey, disagreeing red.  model: a ULIP_PointBERT_partseg (run in eval mode under no_grad, in
    its own precision mode; the training flag is restored); pc [B, N, 3], cls_label [B] or [B, 1], part_label [B, N] as
    validate_partseg takes them.  -> uint8 [B, rows * size, V * size, 3] on the device.  One model call, one predict call, one
    render call for all B x V geometries; nothing is read back to the host."""
    views = views_from_mouse(DEFAULT_VIEWS_MOUSE) if views is None else list(views)
    dev = torch.device("cuda", torch.cuda.current_device())
    pc, cls_label, part_label = (t if t.is_cuda else t.to(dev, non_blocking=True) for t in (pc, cls_label, part_label))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            logits = model(pc, evaluate.to_categorical(cls_label, len(category2part)))          # validate_partseg's one-hot
    finally:
        model.train(was_training)
    with torch.no_grad():
        pred = predict_parts(logits, part_label, category2part)
        B, N = part_label.shape
        V = len(views)
        pal = palette_tensor(palette, pc.device)
        start = _tables(category2part, pc.device)[0][part_label[:, 0].long()]
        layers = [part_colors(part_label, start, pal), part_colors(pred, start, pal)]
        if error_map:
            marks = torch.tensor([DISAGREE, AGREE], dtype=torch.float32, device=pc.device)
            layers.append(marks[(pred.long() == part_label.long()).long()])
        K = len(layers)
        colors = torch.stack(layers, 1)[:, None].expand(B, V, K, N, 3)                        # the same colours under every view
        img = render_balls(camera(pc[..., :3], views, size), colors, size, radius, background)  # [B, V, K, size, size, 3]
        return img.permute(0, 2, 3, 1, 4, 5).reshape(B, K * size, V * size, 3)


def save_png(path, image):
    """image: uint8 [H, W, 3] RGB (tensor or array) -> a PNG file"""
    from PIL import Image
    arr = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"save_png: expected uint8 [H, W, 3], got {arr.dtype} {arr.shape}")
    Image.fromarray(np.ascontiguousarray(arr), "RGB").save(path, format="PNG")
    return path


def parser():
    ap = argparse.ArgumentParser(description="part-segmentation contact sheets of a checkpoint_best.pt (notebook/show_balls.py, "
                                             "show-partseg.sh), one PNG per cloud of the chosen category")
    ap.add_argument("--class_choice", required=True, help="category name, e.g. Chair")
    ap.add_argument("--ballradius", type=int, default=13)
    ap.add_argument("--proj_name", default="ulip2_partseg")
    ap.add_argument("--exp_name", default="run")
    ap.add_argument("--output_dir", default="outputs")
    ap.add_argument("--ckpt", default=None, help="checkpoint_best.pt (default: OUTPUT_DIR/PROJ_NAME/EXP_NAME/checkpoint_best.pt)")
    ap.add_argument("--ulip2", action="store_true")
    ap.add_argument("--num_learnable_prompt_tokens", type=int, default=32)
    ap.add_argument("--class_name_position", default="middle")
    ap.add_argument("--template_init", default="")
    ap.add_argument("--dataset_name", default="shapenetpart")
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--data", required=True, help=".npz: points [M, N, 3] f32, labels [M] (category index), seg [M, N] (part ids) "
                                                  "and optionally parts (the part ranges as a JSON string)")
    ap.add_argument("--parts", default=None, help="JSON file {category: [part ids]} (default: the npz's `parts`)")
    ap.add_argument("--views", default=None, help="mouse fractions 'x,y;x,y;...' as the reference's window reads them "
                                                  "(0.5,0.5: no rotation)")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", required=True, help="directory the PNG files go to")
    return ap


def _parse_views(text):
    if not text:
        return views_from_mouse(DEFAULT_VIEWS_MOUSE)
    return views_from_mouse([tuple(float(v) for v in pair.split(",")) for pair in text.split(";") if pair.strip()])


def _build_model(a):
    from .models import ULIP_models as M
    a.classnames = M.dataset_classnames(a.dataset_name)
    a.task, a.head_type, a.evaluate_3d = "partseg", 0, False
    return M.ULIP_PointBERT_partseg(a).cuda()


def main(argv=None):
    a = parser().parse_args(argv)
    import collections
    with np.load(a.data, allow_pickle=False) as f:
        points, labels, seg = np.ascontiguousarray(f["points"], dtype=np.float32), f["labels"].astype(np.int64), f["seg"].astype(np.int64)
        parts_json = str(f["parts"]) if "parts" in f.files else None
    if a.parts:
        with open(a.parts) as fh:
            category2part = json.load(fh, object_pairs_hook=collections.OrderedDict)
    elif parts_json is not None:
        category2part = json.loads(parts_json, object_pairs_hook=collections.OrderedDict)
    else:
        raise SystemExit("the part ranges are missing: give --parts FILE.json or store `parts` (a JSON string) in the .npz")
    if a.class_choice not in category2part:
        raise SystemExit(f"{a.class_choice!r} is not a category of {list(category2part)}")
    points, seg = points[:, :a.npoints, :3], seg[:, :a.npoints]
    # the reference's sense of "the chosen class": the category of point 0's label (show_balls.py:246-248)
    wanted = np.isin(seg[:, 0], np.asarray(category2part[a.class_choice], dtype=np.int64))
    chosen = np.flatnonzero(wanted)
    if chosen.size == 0:
        print(f'There is no {a.class_choice} in the data!')
        return []
    torch.cuda.set_device(a.gpu)
    from .train import load_prompt_checkpoint
    path = a.ckpt or os.path.join(a.output_dir, a.proj_name, a.exp_name, 'checkpoint_best.pt')
    model = _build_model(a)
    load_prompt_checkpoint(model, torch.load(path, map_location="cpu", weights_only=False))
    os.makedirs(a.out, exist_ok=True)
    views = _parse_views(a.views)
    written = []
    for o in range(0, chosen.size, a.batch_size):
        rows = chosen[o:o + a.batch_size]
        sheets = partseg_sheet(model, torch.from_numpy(points[rows]), torch.from_numpy(labels[rows]), torch.from_numpy(seg[rows]),
                               category2part, views=views, size=a.size, radius=a.ballradius)
        for row, sheet in zip(rows.tolist(), sheets.cpu()):                               # the one transfer of the batch
            written.append(save_png(os.path.join(a.out, f"{a.class_choice}_{row}.png"), sheet))
    print(f"=> wrote {len(written)} pictures to {a.out}")
    return written


if __name__ == "__main__":
    main()
