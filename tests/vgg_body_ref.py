"""Float64 restatement of the VGG-16 body of the weak-paired scripts (004_train_arch{1,2}_weakpaired_autoencoder_vgg.lua):
net_utils.prepro's window and mean subtraction, the public VGG-16 layer list up to fc7 with torch.nn.functional.conv2d, and
the two Dropouts behind fc6 / fc7 (modules 35 and 38) with the masks of include/nvqa_rng.h, taken from
tests/ref_autograd.hash32.  A different formulation from the library's (NCHW, direct convolutions, CHW flatten, no channel
padding, no split-K); anchored to the direct-convolution CPU oracle in tests/test_vgg_body_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from ref_autograd import hash32

CONV_COUT = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
POOL_AFTER = [0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1]
MEAN_RGB = np.array([123.68, 116.779, 103.939], np.float32)  # the ABI's constants are float32
SITE_VGG_FC6, SITE_VGG_FC7 = 10, 11


def raw_images(n, S, seed):
    """uint8 planar RGB [n x 3 x S x S] as /images/<split> stores them"""
    return np.random.default_rng(seed).integers(0, 256, (n, 3, S, S), dtype=np.uint8)


def host_crop(images_u8, xoff, yoff, hw, dtype=np.float32):
    """net_utils.prepro on the host: the hw x hw window at the 0-based origin (xoff, yoff), as float, minus the RGB mean, as
    BGR planes [n x 3 x hw x hw] -- what nvqa_vgg16_fc7 takes (loadim's layout)."""
    win = images_u8[:, :, yoff:yoff + hw, xoff:xoff + hw].astype(dtype)
    win = win - MEAN_RGB.astype(dtype).reshape(1, 3, 1, 1)
    return np.ascontiguousarray(win[:, ::-1])


def dropout_mask(dr, site, n, width):
    """[n x width] multipliers of nvqa_dropout_scale: idx = b * width + j, u = (hash32 >> 8) 2^-24, kept (u >= p) x 1/(1-p)"""
    p = np.float32(dr.p)
    inv_keep = np.float32(1.0) / (np.float32(1.0) - p)
    m = np.zeros((n, width), np.float64)
    for b in range(n):
        for j in range(width):
            u = np.float32(hash32(dr.seed, dr.step, site, b * width + j) >> 8) * np.float32(1.0 / 16777216.0)
            m[b, j] = float(inv_keep) if u >= p else 0.0
    return m


def body_fc7(div, hw, flat, x_bgr, dr=None):
    """module 38's output [n x F] in float64 from preprocessed BGR planes; dr (mode 1): drop6 / drop7 live.
    Returns (features, mask6, mask7); the masks are None without dr."""
    w = torch.from_numpy(np.asarray(flat, np.float64))
    x = torch.from_numpy(np.asarray(x_bgr, np.float64))
    n, off, cin = x.shape[0], 0, 3
    for i, c in enumerate(CONV_COUT):
        co = max(1, c // div)
        W = w[off:off + co * cin * 9].reshape(co, cin, 3, 3); off += co * cin * 9
        b = w[off:off + co]; off += co
        x = F.relu(F.conv2d(x, W, b, padding=1))
        if POOL_AFTER[i]:
            x = F.max_pool2d(x, 2, 2)
        cin = co
    Fw = max(4, 4096 // div)
    x = x.reshape(n, -1)  # CHW flatten: the Caffe order of fc6's columns
    m6 = m7 = None
    if dr is not None and dr.mode:
        m6, m7 = dropout_mask(dr, SITE_VGG_FC6, n, Fw), dropout_mask(dr, SITE_VGG_FC7, n, Fw)
    for k, m in ((x.shape[1], m6), (Fw, m7)):
        W = w[off:off + Fw * k].reshape(Fw, k); off += Fw * k
        b = w[off:off + Fw]; off += Fw
        x = F.relu(x @ W.t() + b)
        if m is not None:
            x = x * torch.from_numpy(m)
    assert off == w.numel()
    return x.numpy(), m6, m7


def body_fc7_raw(div, hw, flat, images_u8, xoff, yoff, dr=None):
    """the whole route in float64: window, mean, body"""
    return body_fc7(div, hw, flat, host_crop(images_u8, xoff, yoff, hw, np.float64), dr)
