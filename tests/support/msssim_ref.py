"""pytorch_msssim 1.0's ssim / ms_ssim (win=None) restated in plain torch (F.conv2d with groups = C, F.avg_pool2d), in the dtype of its inputs:
float64 inputs make it the value and gradient oracle of inv3d_amd.metrics, float32 inputs on the GPU the composite those kernels replace.
Unlike the library it raises on a side shorter than the window (the library skips the smoothing along that axis)."""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss_1d(size=11, sigma=1.5, dtype=torch.float64):
    coords = torch.arange(size, dtype=dtype) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def blur(x, g):
    """The valid separable window, H then W, per channel."""
    c, k = x.shape[1], g.numel()
    g = g.to(x)
    x = F.conv2d(x, g.view(1, 1, k, 1).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, k).repeat(c, 1, 1, 1), groups=c)


def ssim_cs(X, Y, data_range=255, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """(mean ssim, mean cs) per (image, channel), [N, C] each."""
    if min(X.shape[-2:]) < win_size:
        raise ValueError('side below the window')
    g = gauss_1d(win_size, win_sigma, X.dtype)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = blur(X, g), blur(Y, g)
    s11 = blur(X * X, g) - mu1 ** 2
    s22 = blur(Y * Y, g) - mu2 ** 2
    s12 = blur(X * Y, g) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def pool(x):
    """avg_pool2d(2, 2, padding = side % 2, count_include_pad): an odd side pads a zero at both ends, the divisor is always 4."""
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def level_sizes(h, w, levels=5):
    out = [(h, w)]
    for _ in range(levels - 1):
        h, w = (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1
        out.append((h, w))
    return out


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    s, _ = ssim_cs(X, Y, data_range, win_size, win_sigma, K)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    w = torch.tensor(WEIGHTS if weights is None else weights, dtype=X.dtype, device=X.device)
    assert min(X.shape[-2:]) > (win_size - 1) * (2 ** 4)
    mcs = []
    for i in range(w.numel()):
        s, cs = ssim_cs(X, Y, data_range, win_size, win_sigma, K)
        if i < w.numel() - 1:
            mcs.append(torch.relu(cs))
            X, Y = pool(X), pool(Y)
    vals = torch.stack(mcs + [torch.relu(s)], 0)
    v = torch.prod(vals ** w.view(-1, 1, 1), 0)
    return v.mean() if size_average else v.mean(1)
