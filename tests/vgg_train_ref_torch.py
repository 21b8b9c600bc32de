"""Torch model of the VGG-16 body for the fine-tuning tests (protos.cnn:forward / :backward of
004_train_arch{1,2}_weakpaired_autoencoder_vgg.lua), float64 unless told otherwise, with a FIXED-PATTERN form: the ReLU masks,
the max-pool selections and the fc masks (ReLU x Dropout) are inputs.  A tensor multiply applies a mask and a gather on the
unfolded 2 x 2 windows does a selection, so the fixed-pattern network is linear in everything else and autograd through it
is the backward pass that a given pattern defines -- the yardstick for a device whose float32 forward may decide a near-tie
the other way than float64 does.

`free_forward` runs the ordinary network (relu / first-maximum pooling) and returns the pattern it took, with every unit's
margin: |pre-activation| for a ReLU, the gap between the two largest window values for a pool, both relative to the layer's
largest magnitude.  Layout of the flat vectors: nvqa_vgg16_set_weights' (Caffe order)."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

import vgg_body_ref as vref
from vgg_body_ref import CONV_COUT, POOL_AFTER

SGD, SGDM, ADAM = 0, 1, 5  # NVQA_OPT_*


class Drop(collections.namedtuple("Drop", "mode p seed step")):
    """the fields of nvqa_dropout"""


# the cases of the GPU tests (tests/test_gpu_vgg_train.py): (width_div, input_hw, n, S) with the window origin, the seed of the
# images and d(features), and the live drop6 / drop7 of one of them.  tests/test_vgg_train_ref.py checks on the CPU that a
# float32 run of each takes the float64 run's pattern but for a few near-ties.
CASES = {
    "narrow": dict(div=16, hw=32, n=3, S=40, xoff=7, yoff=3, seed=51, dr=Drop(1, 0.5, 77, 3)),  # general loaders, K = 12 at conv5_x
    "half": dict(div=2, hw=32, n=2, S=40, xoff=8, yoff=0, seed=52, dr=None),                    # C_in a multiple of the tiles
    "full": dict(div=1, hw=64, n=2, S=72, xoff=5, yoff=6, seed=53, dr=None),                    # full-width tiles
}
PATTERN_SHARE, NEAR_TIE = 1e-4, 1e-4  # at most this share of a layer's units may differ, each with a margin below NEAR_TIE


def case_inputs(c):
    """(uint8 images, preprocessed float64 crop, d(features)) of a case"""
    img = vref.raw_images(c["n"], c["S"], c["seed"])
    x = vref.host_crop(img, c["xoff"], c["yoff"], c["hw"], np.float64)
    dfeats = np.random.default_rng(c["seed"] + 1000).standard_normal((c["n"], max(4, 4096 // c["div"]))).astype(np.float32)
    return img, x, dfeats


def tensor_names():
    names = []
    for i in range(13):
        names += ["conv%d.w" % i, "conv%d.b" % i]
    return names + ["fc6.w", "fc6.b", "fc7.w", "fc7.b"]


def split(div, hw, flat):
    """the 30 tensors of a flat vector (views): conv W [co, ci, 3, 3], b; fc6 W [F, c5 S S], b; fc7 W [F, F], b"""
    out, off, cin = [], 0, 3
    for c in CONV_COUT:
        co = max(1, c // div)
        out.append(flat[off:off + co * cin * 9].reshape(co, cin, 3, 3)); off += co * cin * 9
        out.append(flat[off:off + co]); off += co
        cin = co
    Fw, s = max(4, 4096 // div), hw // 32
    for k in (cin * s * s, Fw):
        out.append(flat[off:off + Fw * k].reshape(Fw, k)); off += Fw * k
        out.append(flat[off:off + Fw]); off += Fw
    assert off == flat.shape[0]
    return out


def windows(x):
    """[n, C, H, W] -> [n, C, H/2, W/2, 4], the 2 x 2 windows in row-major order"""
    n, c, h, w = x.shape
    return x.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def first_max(x):
    """index (0..3, row-major) of the first maximum of every window: Torch's SpatialMaxPooling rule (argmax returns the first)"""
    return windows(x).argmax(-1)


def fc_masks(n, Fw, dr):
    """the Dropout multipliers behind fc6 / fc7 (ones without a live dropout)"""
    if dr is None or not dr.mode:
        return np.ones((n, Fw)), np.ones((n, Fw))
    return vref.dropout_mask(dr, vref.SITE_VGG_FC6, n, Fw), vref.dropout_mask(dr, vref.SITE_VGG_FC7, n, Fw)


def free_forward(div, hw, flat, x_bgr, dr=None, dtype=torch.float64):
    """the ordinary network.  Returns (features, acts, pattern, margins): acts = the 13 post-ReLU convolution outputs + fc6 +
    fc7 outputs (post-dropout); pattern = {"relu": 13 bool, "sel": 5 int64, "fc": 2 multipliers (ReLU mask x dropout)};
    margins = {"relu": 13, "sel": 5, "fc": 2} relative margins of every unit's decision."""
    w = split(div, hw, torch.as_tensor(np.asarray(flat), dtype=dtype))
    x = torch.as_tensor(np.asarray(x_bgr), dtype=dtype)
    n = x.shape[0]
    acts, pat, mar = [], {"relu": [], "sel": [], "fc": []}, {"relu": [], "sel": [], "fc": []}
    for i in range(13):
        z = F.conv2d(x, w[2 * i], w[2 * i + 1], padding=1)
        pat["relu"].append(z > 0)
        mar["relu"].append(z.abs() / z.abs().max())
        x = F.relu(z)
        acts.append(x)
        if POOL_AFTER[i]:
            win = windows(x)
            top = win.topk(2, -1).values
            pat["sel"].append(win.argmax(-1))
            mar["sel"].append((top[..., 0] - top[..., 1]) / x.max())
            x = F.max_pool2d(x, 2, 2)
    x = x.reshape(n, -1)
    drops = fc_masks(n, w[26].shape[0], dr)
    for k in range(2):
        z = x @ w[26 + 2 * k].t() + w[27 + 2 * k]
        m = (z > 0).to(dtype) * torch.as_tensor(drops[k], dtype=dtype)
        pat["fc"].append(m)
        mar["fc"].append(z.abs() / z.abs().max())
        x = z * m
        acts.append(x)
    return x, acts, pat, mar


def pattern_of(acts, dr=None):
    """the pattern a run took, read off its stored outputs alone (what the device's backward does): ReLU mask = [y > 0], pool
    selection = first maximum of the stored windows, fc multiplier = [y > 0] / keep (a kept, positive unit is a positive y)"""
    acts = [torch.as_tensor(np.asarray(a)) for a in acts]
    s = float(np.float32(1.0) / (np.float32(1.0) - np.float32(dr.p))) if dr is not None and dr.mode else 1.0  # the ABI's float32
    return {"relu": [a > 0 for a in acts[:13]],
            "sel": [first_max(acts[i]) for i in range(13) if POOL_AFTER[i]],
            "fc": [(a > 0).to(torch.float64) * s for a in acts[13:]]}


def fixed_forward(div, hw, w_flat, x_bgr, pat, dtype=torch.float64):
    """the network under a given pattern.  w_flat: a torch vector (may require grad).  Returns (features, acts)."""
    w = split(div, hw, w_flat)
    x = torch.as_tensor(np.asarray(x_bgr), dtype=dtype)
    n, np_, acts = x.shape[0], 0, []
    for i in range(13):
        x = F.conv2d(x, w[2 * i], w[2 * i + 1], padding=1) * pat["relu"][i].to(dtype)
        acts.append(x)
        if POOL_AFTER[i]:
            x = windows(x).gather(-1, pat["sel"][np_].unsqueeze(-1)).squeeze(-1)
            np_ += 1
    x = x.reshape(n, -1)
    for k in range(2):
        x = (x @ w[26 + 2 * k].t() + w[27 + 2 * k]) * pat["fc"][k].to(dtype)
        acts.append(x)
    return x, acts


def l2norm_backward(f, dy):
    """nn.L2Normalize:updateGradInput (misc/L2Normalize.lua:22-40) in closed form: (r^2 I - f f^T) / r^3 dy, row by row"""
    r = np.sqrt((f * f).sum(1, keepdims=True))
    return dy / r - f * (f * dy).sum(1, keepdims=True) / r ** 3


def fixed_backward(div, hw, flat, x_bgr, pat, dfeats, through_l2norm=False, dtype=torch.float64):
    """d(sum(features . dfeats))/d(weights) under the pattern, as a flat numpy vector of `dtype`.  through_l2norm: dfeats is
    d/d(f^) and the features are row-normalised first."""
    w = torch.tensor(np.asarray(flat), dtype=dtype, requires_grad=True)
    f, _ = fixed_forward(div, hw, w, x_bgr, pat, dtype)
    if through_l2norm:
        f = f / f.pow(2).sum(1, keepdim=True).sqrt()
    (f * torch.as_tensor(np.asarray(dfeats), dtype=dtype)).sum().backward()
    return w.grad.numpy()


def pattern_diff(pa, pb, margins):
    """per layer: (name, units, differing units, largest margin among the differing units) of two patterns; margins are those
    of the run that took pa"""
    out = []
    for kind in ("relu", "sel", "fc"):
        for i, (a, b) in enumerate(zip(pa[kind], pb[kind])):
            d = (a != 0) != (b != 0) if kind != "sel" else a != b
            m = margins[kind][i][d]
            out.append(("%s%d" % (kind, i), d.numel(), int(d.sum()), float(m.max()) if m.numel() else 0.0))
    return out


class ScaledRule:
    """The lrs forms of misc/optim_updates.lua (sgd :4-10, sgdm :12-24, adam :78-111) with one scale for every element, in the
    scripts' order: g += wd (x scale) when wd > 0, clamp when clamp > 0, the rule.  float64.  update() returns
    (x_new, |x|_2, count(|lr g| >= 0.01 |x|)) with x before the update and g after wd and clamp."""

    def __init__(self, rule, n):
        self.rule, self.t = rule, 0
        self.m, self.v = np.zeros(n), np.zeros(n)

    def update(self, x, g, lr, alpha, beta, eps, wd, clamp, scale):
        x, g = np.asarray(x, np.float64), np.asarray(g, np.float64).copy()
        if wd != 0:
            g += wd * (x * scale)
        if clamp > 0:
            g = np.clip(g, -clamp, clamp)
        norm, count = float(np.sqrt((x * x).sum())), int((np.abs(g * lr) >= np.abs(x) * 0.01).sum())
        if self.rule == SGD:
            x = x - lr * g * scale
        elif self.rule == SGDM:
            self.m = alpha * self.m + lr * g * scale
            x = x - self.m
        else:
            self.m = alpha * self.m + (1 - alpha) * g
            self.v = beta * self.v + (1 - beta) * g * g
            self.t += 1
            step = lr * np.sqrt(1 - beta ** self.t) / (1 - alpha ** self.t)
            x = x - step * (self.m / (np.sqrt(self.v) + eps)) * scale
        return x, norm, count
