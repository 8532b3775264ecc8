"""What csrc/cloud_augment.hip is written to compute, restated in numpy / plain Python: the stages of ppt_cloud_augment_f32 one
float operation at a time (numpy's elementwise operations never fuse a product into a sum), and the device draws of
ppt_cloud_draws_aug as a function of the counter.  tests/golden/make_golden_augment.py pins the stage restatements to the reference's
functions while it generates tests/golden/g_augment.npz; tests/test_augment_gpu.py compares the kernels with both."""
import math

import numpy as np

from test_datapipe_cpu import philox4x32_10

F32, F64 = np.float32, np.float64


# ---- the stages, in the kernel's order of operations: p [n, 3] float32 -> a new [n, 3] float32 ---------------------------------------
def dropout(p, mask):
    out = p.copy()
    out[np.asarray(mask).astype(bool)] = p[0]                 # row 0 as it is at this stage (it can only be replaced by itself)
    return out


def scale(p, s):
    return (p.astype(F64) * F64(s)).astype(F32)


def shift(p, t):
    return (p.astype(F64) + np.asarray(t, F64)).astype(F32)


def rotate(p, R):
    x, y, z = (p[:, c].astype(F64) for c in range(3))
    R = np.asarray(R, F64)
    return np.stack([((x * R[0, c] + y * R[1, c]) + z * R[2, c]).astype(F32) for c in range(3)], axis=1)


def jitter(p, noise):
    return (np.asarray(noise, F64) + p.astype(F64)).astype(F32)


def affine(p, sc, sh):
    return (p.astype(F64) * np.asarray(sc, F64) + np.asarray(sh, F64)).astype(F32)


def height(p):
    return np.concatenate([p, (p[:, 1:2] - p[:, 1:2].min()).astype(F32)], axis=1)


STAGE_FN = {"dropout": dropout, "scale": scale, "shift": shift, "rotate": rotate, "jitter": jitter, "affine": affine}


def chain(p, stages, with_height=False):
    """stages: (kernel stage name, parameters of ONE cloud ...) in order"""
    for st in stages:
        p = STAGE_FN[st[0]](p, *st[1:])
    return height(p) if with_height else p


def ulp32(x):
    """the spacing of float32 at |x| (for the rotation's bound: one ulp of the row's largest coordinate magnitude)"""
    return np.spacing(np.abs(np.asarray(x, F32)))


# ---- the device draws (include/ppt_hip.h, ppt_cloud_draws_aug): counter (index, epoch, slot, block), key = seed ----------------------
SLOT = dict(ratio=4, mask=5, scale=6, shift=7, perturb=8, rotate=9, noise=10)
DEFAULTS = dict(max_dropout=0.875, scale_low=0.8, scale_high=1.25, shift_range=0.1, angle_sigma=0.06, angle_clip=0.18,
                jitter_sigma=0.01, jitter_clip=0.05)
TWO_PI = 2 * math.pi


def u53(hi, lo):
    return float(((hi >> 5) << 26) | (lo >> 6)) * (1.0 / 9007199254740992.0)


def uniforms(w):
    return u53(w[0], w[1]), u53(w[2], w[3])


def box_muller(w):
    u1, u2 = uniforms(w)
    r, th = math.sqrt(-2.0 * math.log(1.0 - u1)), TWO_PI * u2
    return r * math.cos(th), r * math.sin(th)


def clip(v, c):
    return min(max(v, -c), c)


def matmul3(A, B):
    """each entry a sum of three products, left to right, every step rounded in float64"""
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def device_draws(index, epoch, seed, n, **mag):
    """-> dict for ONE sample: ratio, u [n] (the mask's uniforms), mask [n] u8, scale, shift [3], z [3] (the normals behind the
    angles), angles [3], perturb [3, 3], u_angle, angle, rotate [3, 3], zn [n * 3] (the normals behind the noise), noise [n, 3]"""
    m = dict(DEFAULTS, **mag)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    ix = index & 0xFFFFFFFF

    def block(slot, j):
        return philox4x32_10((ix, epoch, slot, j), key)
    d = {}
    d["ratio"] = uniforms(block(SLOT["ratio"], 0))[0] * m["max_dropout"]
    u = [x for j in range((n + 1) // 2) for x in uniforms(block(SLOT["mask"], j))][:n]
    d["u"] = np.array(u)
    d["mask"] = (d["u"] <= d["ratio"]).astype(np.uint8)
    d["scale"] = m["scale_low"] + (m["scale_high"] - m["scale_low"]) * uniforms(block(SLOT["scale"], 0))[0]
    d["shift"] = np.array([-m["shift_range"] + (m["shift_range"] - -m["shift_range"]) * uniforms(block(SLOT["shift"], c))[0]
                           for c in range(3)])
    z = list(box_muller(block(SLOT["perturb"], 0))) + [box_muller(block(SLOT["perturb"], 1))[0]]
    a = [clip(m["angle_sigma"] * v, m["angle_clip"]) for v in z]
    c, s = [math.cos(v) for v in a], [math.sin(v) for v in a]
    Rx = [[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]]
    Ry = [[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]]
    Rz = [[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]
    d["z"], d["angles"], d["perturb"] = np.array(z), np.array(a), np.array(matmul3(Rz, matmul3(Ry, Rx)))
    d["u_angle"] = uniforms(block(SLOT["rotate"], 0))[0]
    d["angle"] = d["u_angle"] * TWO_PI
    ca, sa = math.cos(d["angle"]), math.sin(d["angle"])
    d["rotate"] = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    zn = [x for j in range((n * 3 + 1) // 2) for x in box_muller(block(SLOT["noise"], j))][:n * 3]
    d["zn"] = np.array(zn)
    d["noise"] = np.array([clip(m["jitter_sigma"] * v, m["jitter_clip"]) for v in zn]).reshape(n, 3)
    return d
