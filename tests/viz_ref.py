"""Shared by tests/test_viz_cpu.py and tests/test_viz_gpu.py: numpy restatements of what ppt_amd/viz.py and csrc/render.hip
compute -- the ball renderer as the sequential loop include/ppt_hip.h describes (and a vectorised twin for the larger cases), the
camera of show_balls.py:73-75, 97-119 and the category-masked arg-max of show_balls.py:256-262 -- and the seeded cases both test
files use."""
import collections
import functools

import numpy as np

# ShapeNetPart's ranges (show_balls.py:32-35)
CATEGORY2PART = collections.OrderedDict([
    ('Airplane', [0, 1, 2, 3]), ('Bag', [4, 5]), ('Cap', [6, 7]), ('Car', [8, 9, 10, 11]), ('Chair', [12, 13, 14, 15]),
    ('Earphone', [16, 17, 18]), ('Guitar', [19, 20, 21]), ('Knife', [22, 23]), ('Lamp', [24, 25, 26, 27]), ('Laptop', [28, 29]),
    ('Motorbike', [30, 31, 32, 33, 34, 35]), ('Mug', [36, 37]), ('Pistol', [38, 39, 40]), ('Rocket', [41, 42, 43]),
    ('Skateboard', [44, 45, 46]), ('Table', [47, 48, 49])])


# ---- the renderer -------------------------------------------------------------------------------------------------------------
def pattern(radius):
    """[(dx, dy, dz, s)] for every offset with dx^2 + dy^2 < r^2 (strictly), r = max(radius, 1): dz = sqrt(double(r^2 - dx^2 -
    dy^2)), s = dz / r"""
    r = max(int(radius), 1)
    out = []
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            if dx * dx + dy * dy < r * r:
                dz = float(np.sqrt(np.float64(r * r - dx * dx - dy * dy)))
                out.append((dx, dy, dz, dz / r))
    return r, out


def _shade(win, z2, s, ixyz, colors, r, background):
    """winner map, its depth offer and shade per pixel -> [K, H, W, 3] uint8, every step in double and in the stated order"""
    K = colors.shape[0]
    H, W = win.shape
    out = np.empty((K, H, W, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    hit = win >= 0
    if hit.any():
        zmin = np.float64(int(ixyz[:, 2].min()) - r)
        zmax = np.float64(int(ixyz[:, 2].max()) + r)
        intensity = np.minimum(1.0, (z2[hit].astype(np.float64) - zmin) / (zmax - zmin) * 0.7 + 0.3)
        for k in range(K):
            c = colors[k][win[hit]].astype(np.float64)                       # [pixels, 3]
            out[k][hit] = (s[hit][:, None] * c * intensity[:, None]).astype(np.uint8)
    return out


def render_sequential(ixyz, colors, H, W, radius, background):
    """The rule as a loop: the points in order, a strict `<` depth test.  ixyz [n, 3] int, colors [K, n, 3] f32 ->
    (pictures [K, H, W, 3] uint8, winner [H, W] int64 with -1 where nobody reached)"""
    r, pat = pattern(radius)
    win = np.full((H, W), -1, np.int64)
    zbuf = np.zeros((H, W), np.int64)
    shade = np.zeros((H, W), np.float64)
    for i in range(ixyz.shape[0]):
        x, y, z = (int(v) for v in ixyz[i])
        for dx, dy, dz, s in pat:
            px, py = x + dx, y + dy
            if px < 0 or px >= H or py < 0 or py >= W:
                continue
            z2 = int(float(z) + dz)                                          # int(): toward zero
            if win[px, py] < 0 or zbuf[px, py] < z2:
                win[px, py], zbuf[px, py], shade[px, py] = i, z2, s
    return _shade(win, zbuf, shade, ixyz, colors, r, background), win


def render_vectorised(ixyz, colors, H, W, radius, background):
    """The same pictures from one np.maximum.at over 64-bit keys (z2 biased to unsigned) << 32 | (0xFFFFFFFF - i) per pattern
    entry"""
    r, pat = pattern(radius)
    n = ixyz.shape[0]
    keys = np.zeros((H, W), np.uint64)
    x, y, z = (ixyz[:, k].astype(np.int64) for k in range(3))
    low = (0xFFFFFFFF - np.arange(n, dtype=np.int64)).astype(np.uint64)
    side = 2 * r - 1
    s_table = np.zeros((side, side), np.float64)
    for dx, dy, dz, s in pat:
        s_table[dx + r - 1, dy + r - 1] = s
        px, py = x + dx, y + dy
        ok = (px >= 0) & (px < H) & (py >= 0) & (py < W)
        z2 = np.trunc(z.astype(np.float64) + dz).astype(np.int64)
        key = ((z2 + (1 << 31)).astype(np.uint64) << np.uint64(32)) | low
        np.maximum.at(keys, (px[ok], py[ok]), key[ok])
    hit = keys != 0
    win = np.where(hit, 0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    z2 = (keys >> np.uint64(32)).astype(np.int64) - (1 << 31)
    shade = np.zeros((H, W), np.float64)
    rows, cols = np.nonzero(hit)
    shade[rows, cols] = s_table[rows - x[win[rows, cols]] + r - 1, cols - y[win[rows, cols]] + r - 1]
    return _shade(win, z2, shade, ixyz, colors, r, background), win


#            name        H    W    n    r   depth range
RENDER_CASES = collections.OrderedDict([
    ("small", (70, 45, 40, 5, 60)),
    ("wide_ball", (96, 96, 60, 13, 60)),                  # the ball is wider than a 16-pixel unit of the shading pass
    ("one_entry", (33, 33, 65, 1, 60)),                   # r = 1: a single-entry pattern
    ("deep", (130, 70, 120, 6, 10 ** 6)),
    ("empty", (64, 64, 0, 4, 60)),
    ("single", (40, 50, 1, 7, 60)),
    ("covered", (96, 96, 513, 13, 60)),                   # heavy overlap; more points than one chunk of the kernel's walk
])
BACKGROUNDS = ((255, 255, 255), (12, 40, 200))


def make_geometry(H, W, n, r, depth, seed, K=2):
    """Seeded points and colours with everything the rule has to get right: centres from [-r - 2, size + r + 2) so that balls
    straddle every edge and some are off-screen, negative depths (truncation toward zero), exact duplicates and equal depths (the
    tie rule).  -> (ixyz [n, 3] int32, colors [K, n, 3] f32)"""
    rng = np.random.RandomState(seed)
    ixyz = np.stack([rng.randint(-r - 2, H + r + 2, n), rng.randint(-r - 2, W + r + 2, n), rng.randint(-depth, depth + 1, n)],
                    -1).astype(np.int32).reshape(n, 3)
    if n >= 8:
        dup = n // 8
        ixyz[0, 2] = -depth                                                      # the range's lower end is present
        head = ixyz[:n - 2 * dup]
        on = np.flatnonzero((head[:, 0] >= 0) & (head[:, 0] < H) & (head[:, 1] >= 0) & (head[:, 1] < W))
        assert on.size >= 4
        src = on[rng.randint(0, on.size, dup)]
        ixyz[n - dup:] = ixyz[src]                                               # exact duplicates, at higher indices
        ixyz[n - 2 * dup:n - dup, 2] = ixyz[src, 2]                              # equal depths at other places ...
        ixyz[n - 2 * dup:n - dup, :2] = ixyz[src, :2] + rng.randint(-2, 3, (dup, 2))          # ... overlapping their twins
    elif n:
        ixyz[0] = (H - 3, 2, -7)                                                 # a lone ball across two edges
    colors = (rng.rand(K, n, 3) * 255.0).astype(np.float32)
    if n:
        colors[:, 0] = 255.0
    return ixyz, colors


@functools.lru_cache(maxsize=None)
def render_case(name, seed=5, K=2):
    """-> dict(ixyz, colors, H, W, r, win, pictures {background: [K, H, W, 3] uint8}): computed once, read by every test"""
    H, W, n, r, depth = RENDER_CASES[name]
    ixyz, colors = make_geometry(H, W, n, r, depth, seed, K)
    pics = {}
    for bg in BACKGROUNDS:
        pics[bg], win = render_vectorised(ixyz, colors, H, W, r, bg)
        pics[bg].setflags(write=False)
    for a in (ixyz, colors, win):
        a.setflags(write=False)
    return dict(ixyz=ixyz, colors=colors, H=H, W=W, r=r, win=win, pictures=pics)


# ---- the camera ---------------------------------------------------------------------------------------------------------------
def camera(xyz, views, size, zoom=1.0):
    """show_balls.py:73-75, 97-119 per cloud and view, in float64 numpy.  xyz [B, N, 3], views [(xangle, yangle)]
    -> (ixyz [B, V, N, 3] int32, the float64 values before truncation)"""
    out = np.empty((xyz.shape[0], len(views), xyz.shape[1], 3), np.float64)
    for b in range(xyz.shape[0]):
        p = xyz[b].astype(np.float64)
        p = p - p.mean(axis=0)
        radius = ((p ** 2).sum(axis=-1) ** 0.5).max()
        p /= (radius * 2.2) / size
        for v, (xangle, yangle) in enumerate(views):
            rotmat = np.eye(3)
            rotmat = rotmat.dot(np.array([[1.0, 0.0, 0.0], [0.0, np.cos(xangle), -np.sin(xangle)], [0.0, np.sin(xangle), np.cos(xangle)]]))
            rotmat = rotmat.dot(np.array([[np.cos(yangle), 0.0, -np.sin(yangle)], [0.0, 1.0, 0.0], [np.sin(yangle), 0.0, np.cos(yangle)]]))
            rotmat *= zoom
            out[b, v] = p.dot(rotmat) + [size / 2, size / 2, 0]
    return out.astype('int32'), out


def in_band(values, width=1e-9):
    """coordinates whose float64 value lies within `width` of an integer: there two evaluation orders may truncate differently"""
    return np.abs(values - np.round(values)) < width


# ---- the masked arg-max -------------------------------------------------------------------------------------------------------
def predict_parts(logits, anchor, c2p=CATEGORY2PART):
    """show_balls.py:256-262: logits [B, N, P], anchor [B] -> [B, N] int32; -1 for an anchor that is no part id"""
    by_part = {p: parts for parts in c2p.values() for p in parts}
    out = np.full(logits.shape[:2], -1, np.int32)
    for b in range(logits.shape[0]):
        parts = by_part.get(int(anchor[b]))
        if parts is not None:
            out[b] = np.argmax(logits[b][:, parts[0]:parts[0] + len(parts)], axis=-1) + parts[0]
    return out
