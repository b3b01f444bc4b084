"""The specification of SSIM / MS-SSIM, restated twice in float64:

    taps        g[i] = exp(-(i - win // 2)^2 / (2 sigma^2)), normalised to sum 1 in fp32
    C1, C2      (K1 R)^2, (K2 R)^2
    mu_x        F(X): the separable filter over VALID positions only, along H and then along W
    s_xx, s_xy  F(X X) - mu_x^2,  F(X Y) - mu_x mu_y
    cs          (2 s_xy + C2) / (s_xx + s_yy + C2)
    ssim        (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs
    per channel the mean over the valid region; SSIM = mean over channels (relu first when nonnegative)
    next scale  avg_pool2d(2, padding = size % 2): divisor 4, output side size // 2 + size % 2
    MS-SSIM     prod_s relu(v_s)^w_s per channel, v_s = cs on the first four scales and ssim on the last; mean

`*_torch` uses torch.nn.functional.conv2d (its autograd is the reference gradient), `*_scipy` uses
scipy.ndimage.correlate1d and numpy slicing and shares no code with it.  Images are [3, H, W] here."""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def taps(win=11, sigma=1.5):
    """fp32 taps, as a float32 numpy array."""
    c = torch.arange(win, dtype=torch.float32) - win // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).numpy()


def pooled_side(size):
    return size // 2 + size % 2


def pooled_sizes(h, w, levels=5):
    out = [(h, w)]
    for _ in range(levels - 1):
        h, w = pooled_side(h), pooled_side(w)
        out.append((h, w))
    return out


# ------------------------------------------------------------------------------------------------------ torch, float64
def _filter_torch(x, g):  # x [1, C, H, W]
    c = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)


def scale_torch(x, y, g, c1, c2):
    """per-channel (mean ssim, mean cs) of [1, C, H, W] images"""
    mx, my = _filter_torch(x, g), _filter_torch(y, g)
    sxx = _filter_torch(x * x, g) - mx * mx
    syy = _filter_torch(y * y, g) - my * my
    sxy = _filter_torch(x * y, g) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ssim = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
    return ssim.flatten(2).mean(-1)[0], cs.flatten(2).mean(-1)[0]


def pool_torch(x):
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def _prep(x, dtype):
    return x.to(dtype)[None] if x.dim() == 3 else x.to(dtype)


def ssim_torch(x, y, data_range=1.0, win=11, sigma=1.5, K=(0.01, 0.03), nonnegative=False, dtype=torch.float64):
    """x, y: [3, H, W] tensors -> (value, per-channel values, per-channel cs means)"""
    g = torch.from_numpy(taps(win, sigma)).to(dtype).to(x.device)
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    s, cs = scale_torch(_prep(x, dtype), _prep(y, dtype), g, c1, c2)
    if nonnegative:
        s = torch.relu(s)
    return s.mean(), s, cs


def ms_ssim_torch(x, y, data_range=1.0, win=11, sigma=1.5, weights=None, K=(0.01, 0.03), dtype=torch.float64):
    """-> (value, per-channel values, [5, 3] ssim means, [5, 3] cs means)"""
    g = torch.from_numpy(taps(win, sigma)).to(dtype).to(x.device)
    w = torch.tensor(WEIGHTS if weights is None else weights, dtype=dtype, device=x.device)
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    x, y = _prep(x, dtype), _prep(y, dtype)
    all_s, all_cs = [], []
    for i in range(len(w)):
        s, cs = scale_torch(x, y, g, c1, c2)
        all_s.append(s)
        all_cs.append(cs)
        if i + 1 < len(w):
            x, y = pool_torch(x), pool_torch(y)
    v = torch.stack([torch.relu(c) for c in all_cs[:-1]] + [torch.relu(all_s[-1])])  # [5, 3]
    per_channel = torch.prod(v ** w.view(-1, 1), dim=0)
    return per_channel.mean(), per_channel, torch.stack(all_s), torch.stack(all_cs)


def loss_value_and_grad(kind, x, y, **kw):
    """float64 value and gradient (to x) of 1 - ssim / 1 - ms_ssim of [3, H, W] images"""
    x = x.detach().to(torch.float64).requires_grad_(True)
    fn = ssim_torch if kind == "ssim" else ms_ssim_torch
    loss = 1 - fn(x, y.detach().to(torch.float64), **kw)[0]
    loss.backward()
    return float(loss), x.grad


# ------------------------------------------------------------------------------------------------------ scipy, float64
def _filter_scipy(a, g):  # a [C, H, W]
    from scipy.ndimage import correlate1d
    half = len(g) // 2
    a = correlate1d(a, g, axis=1, mode="constant")[:, half:a.shape[1] - half]
    return correlate1d(a, g, axis=2, mode="constant")[:, :, half:a.shape[2] - half]


def scale_scipy(x, y, g, c1, c2):
    mx, my = _filter_scipy(x, g), _filter_scipy(y, g)
    sxx = _filter_scipy(x * x, g) - mx * mx
    syy = _filter_scipy(y * y, g) - my * my
    sxy = _filter_scipy(x * y, g) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ssim = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
    return ssim.reshape(ssim.shape[0], -1).mean(1), cs.reshape(cs.shape[0], -1).mean(1)


def pool_scipy(a):
    c, h, w = a.shape
    p = np.zeros((c, 2 * pooled_side(h), 2 * pooled_side(w)), dtype=a.dtype)
    p[:, h % 2:h % 2 + h, w % 2:w % 2 + w] = a  # the padding that is read is the leading row / column
    return (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4


def ssim_scipy(x, y, data_range=1.0, win=11, sigma=1.5, K=(0.01, 0.03), nonnegative=False):
    g = taps(win, sigma).astype(np.float64)
    s, cs = scale_scipy(np.asarray(x, np.float64), np.asarray(y, np.float64), g, (K[0] * data_range) ** 2,
                        (K[1] * data_range) ** 2)
    if nonnegative:
        s = np.maximum(s, 0)
    return s.mean(), s, cs


def ms_ssim_scipy(x, y, data_range=1.0, win=11, sigma=1.5, weights=None, K=(0.01, 0.03)):
    g = taps(win, sigma).astype(np.float64)
    w = np.asarray(WEIGHTS if weights is None else weights, np.float64)
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    all_s, all_cs = [], []
    for i in range(len(w)):
        s, cs = scale_scipy(x, y, g, c1, c2)
        all_s.append(s)
        all_cs.append(cs)
        if i + 1 < len(w):
            x, y = pool_scipy(x), pool_scipy(y)
    v = np.maximum(np.stack(all_cs[:-1] + [all_s[-1]]), 0)
    per_channel = np.prod(v ** w[:, None], axis=0)
    return per_channel.mean(), per_channel, np.stack(all_s), np.stack(all_cs)


# ------------------------------------------------------------------------------------------------------------ pictures
def picture(kind, h, w, seed=0):
    """(prediction, target) as float32 [3, H, W] tensors in [0, 1]"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    if kind == "smooth":
        t = torch.stack([0.5 + 0.4 * torch.sin(6.0 * xx + 3.0 * yy), 0.5 + 0.4 * torch.cos(5.0 * yy - 2.0 * xx),
                         0.3 + 0.5 * xx * yy])
        p = (t + 0.03 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    elif kind == "noise":
        t = torch.rand(3, h, w, generator=g)
        p = torch.rand(3, h, w, generator=g)
    elif kind == "flat":  # flat black and white regions: sigma ~ 0, the variances are differences of near-equal numbers
        t = ((xx * 5).floor() + (yy * 3).floor()).remainder(2).expand(3, h, w).clone()
        p = t.clone()
        p[:, : h // 2] = (p[:, : h // 2] * 0.96 + 0.01)
        p[:, :, w // 3: w // 3 + 7] = 1 - p[:, :, w // 3: w // 3 + 7]
    elif kind == "anti":  # anti-correlated noise: negative cs on the coarse scales, the relu cuts
        t = torch.rand(3, h, w, generator=g)
        p = 1 - t
    elif kind == "fine_anti":  # fine noise anti-correlated between the images on a shared smooth base: cs is clearly
        # negative at scale 0 and near 1 on the coarse scales (a generator of its own: the base draws from g)
        base = 0.6 * picture("smooth", h, w, seed)[1] + 0.2
        n = torch.rand(3, h, w, generator=torch.Generator().manual_seed(seed)) - 0.5
        p, t = base + 0.2 * n, base - 0.2 * n
    else:
        raise ValueError(kind)
    return p.float().contiguous(), t.float().contiguous()
