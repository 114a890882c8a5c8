"""Shared inputs of the FID tests and of tools/make_golden_fid.py: the synthetic InceptionV3 state dict (23.9 M values rebuilt from
oracle.fill.hash_tensor, so the golden file holds expected outputs only), the hash-filled image sets and feature sets, and float64
conv / BatchNorm arithmetic on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill

RESIZE_SHAPES = ((32, 32), (48, 64), (299, 299), (300, 450))      # uint8 inputs of the resize cases (B = 1 each)
EXTRACT_CASES = (("a", 2, 32, 32), ("b", 1, 48, 64))              # (tag, B, H, W) of the whole-extractor cases
METRIC_CASES = ((64, 300, 257), (192, 800, 801))                  # (D, N1, N2) of the fid_statistics cases
ISC_SHAPE = (103, 1008)
E2E_N, E2E_HW, E2E_ISC_N, E2E_ISC_SPLITS = 300, 32, 40, 4
FEATURES = ("64", "192", "768", "2048", "logits_unbiased", "logits")


def sub_idx(n, step=7):
    """every 7th index plus the last: the rows / columns of a resize result the golden file keeps"""
    idx = list(range(0, n, step))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return np.array(idx)


def synthetic_state_dict(shapes):
    """Conv and fc weights uniform at scale sqrt(6 / fan_in) (activations neither die nor explode through 94 ReLU units), BatchNorm
    gamma 1 + 0.1 u, beta and running mean 0.1 u, running variance in [0.5, 1.5]."""
    sd = {}
    for name, shape in shapes.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[name] = torch.tensor(0, dtype=torch.long)
        elif name.endswith("conv.weight") or name == "fc.weight":
            sd[name] = fill.hash_tensor(shape, name, (6.0 / int(np.prod(shape[1:]))) ** 0.5)
        elif name.endswith("bn.weight"):
            sd[name] = 1.0 + fill.hash_tensor(shape, name, 0.1)
        elif name.endswith("running_var"):
            sd[name] = 1.0 + fill.hash_tensor(shape, name, 0.5)
        else:                                  # bn.bias, bn.running_mean, fc.bias
            sd[name] = fill.hash_tensor(shape, name, 0.1)
    return sd


def images_u8(shape, tag):
    """uint8 images from the hash stream: a smooth ramp plus noise, so the resize sees gradients and the network sees structure"""
    u = fill.hash_tensor(shape, tag, 1.0, torch.float64)
    B, C, H, W = shape
    yy = torch.linspace(0, 1, H, dtype=torch.float64)[None, None, :, None]
    xx = torch.linspace(0, 1, W, dtype=torch.float64)[None, None, None, :]
    ph = fill.hash_tensor((B, C, 1, 1), tag + ".phase", 1.0, torch.float64)
    v = 128 + 70 * torch.sin(6.0 * (yy + ph) + 3.0 * xx * (1 + ph)) + 57 * u
    return v.round().clamp(0, 255).to(torch.uint8)


def e2e_sets():
    """the two image sets of the end-to-end FID case: the second is darker and noisier"""
    a = images_u8((E2E_N, 3, E2E_HW, E2E_HW), "fid.e2e.a")
    b = images_u8((E2E_N, 3, E2E_HW, E2E_HW), "fid.e2e.b")
    b = (b.double() * 0.8 + 25 * fill.hash_tensor(b.shape, "fid.e2e.b.n", 1.0, torch.float64)).round().clamp(0, 255).to(torch.uint8)
    return a, b


def metric_features(D, N, tag):
    """[N, D] float64 features with correlated columns and distinct means"""
    z = fill.hash_tensor((N, D), tag, 1.0, torch.float64)
    mix = fill.hash_tensor((D, D), tag + ".mix", 1.0 / D ** 0.5, torch.float64) + torch.eye(D, dtype=torch.float64)
    return (z @ mix + fill.hash_tensor((D,), tag + ".mu", 0.5, torch.float64)).numpy()


def isc_logits():
    return fill.hash_tensor(ISC_SHAPE, "fid.isc.logits", 4.0, torch.float32)


def mean_cov64(x):
    x = np.asarray(x, np.float64)
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def conv_bn_relu64(x, w, gamma, beta, mean, var, stride, pad, eps=1e-3):
    """plain float64 conv -> eval BatchNorm -> ReLU on NCHW tensors"""
    y = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad)
    y = (y - mean.double()[None, :, None, None]) / torch.sqrt(var.double()[None, :, None, None] + eps)
    y = y * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]
    return F.relu(y)
