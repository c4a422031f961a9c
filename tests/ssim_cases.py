"""Helpers of the float64 tests of the piqa-style SSIM / MS-SSIM (csrc/ssim.hip: nd_ssim, nd_ms_ssim, nd_ssim_loss_grad), shared by
tests/test_ssim_float64_host.py (CPU gates) and tests/test_ssim_float64.py (GPU).

* a restatement of oracle/losses.py that takes a dtype and a dict of knobs, each knob one planted error.  The window is always the
  fp32-rounded taps cast to the working dtype: piqa holds its kernel in fp32 and write_window() uploads fp32 taps, so float64 on
  float64 taps would be another function (by how much: tap_distance());
* regimes: deterministic generators of image-like pairs (x, y), x the generated image that is differentiated;
* shapes: the smallest at which each mechanism has an edge (forward tile 32 x 32 on the valid map, backward tile 16 x 16 on the
  image, ceil-mode halving between the five scales);
* edge classes: a pixel's class is (min(d_y, 10), min(d_x, 10)), d the distance to the nearest edge along that axis: 121 classes of
  homogeneous window coverage.  The corner class is touched by one window with weight g0^2 ~ 1e-6, so its gradient is ~1e-6 of the
  interior's and no norm over the whole image sees it: every figure of a gradient here is taken per class.

References.  R64 is the restatement in float64, R32 the same in torch fp32 on the CPU.  A score is held to
max(10 |R32 - R64|, 4 * 2^-24) per sample, a gradient class to 10 x R32's own figure for that class: the factor 10 is the one
test_f32_exact.py uses for HIP against a torch fp32 restatement, 2^-24 the fp32 spacing below 1.

Figures of a gradient are taken per sample: the samples of a batch are of different regimes, whose gradients differ by orders of
magnitude (a dark image divides by mu^2 + c1 ~ 1e-3), and one maximum over the batch would hold every sample to the darkest one's
scale."""
import functools
import zlib

import torch
import torch.nn.functional as F

WINDOW, SIGMA = 11, 1.5
K1, K2 = 0.01, 0.03
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WEIGHT = 0.7                      # the loss weight of every nd_ssim_loss_grad call here
REACH = WINDOW - 1                # 10: a pixel this far from every edge is covered by all 121 windows
NCLASS = (REACH + 1) ** 2
FACTOR = 10.0
SCORE_FLOOR = 4 * 2.0 ** -24
CLASS_BAR_CAP = 0.1               # no class bar may be wider than this on any case (test_ssim_float64_host.py asserts it from R32)

FORWARD_KNOBS = ("c1_unsquared", "c2_unsquared", "last_cs", "weights_swapped", "pool_div4", "mean_full", "no_relu")
MS_ONLY_KNOBS = ("last_cs", "weights_swapped", "pool_div4", "no_relu")


# ---------------------------------------------------------------------------- the restatement

def taps(dtype, exact=False):
    """the 11 taps: computed in fp32 as piqa and write_window() do and cast to dtype (exact: computed in dtype, for tap_distance)"""
    d = dtype if exact else torch.float32
    k = torch.arange(WINDOW, dtype=d) - (WINDOW - 1) / 2
    k = torch.exp(-(k ** 2) / (2 * SIGMA ** 2))
    return (k / k.sum()).to(dtype)


def _filter(x, g):
    c = x.size(1)
    kh = g.view(1, 1, -1, 1).repeat(c, 1, 1, 1)
    kw = g.view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    return F.conv2d(F.conv2d(x, kh, groups=c), kw, groups=c)


def ssim_maps(x, y, knobs=None, exact_taps=False):
    knobs = knobs or {}
    g = taps(x.dtype, exact_taps)
    c1 = K1 if knobs.get("c1_unsquared") else (K1 * 1.0) ** 2
    c2 = K2 if knobs.get("c2_unsquared") else (K2 * 1.0) ** 2
    mu_x, mu_y = _filter(x, g), _filter(y, g)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    s_xx = _filter(x * x, g) - mu_xx
    s_yy = _filter(y * y, g) - mu_yy
    s_xy = _filter(x * y, g) - mu_xy
    cs = (2 * s_xy + c2) / (s_xx + s_yy + c2)
    ss = (2 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return ss, cs


def _mean(m, start, shape, knobs):
    """mean of a valid map over the dims from `start` on (mean_full: divided by the image's pixels instead of the map's)"""
    if knobs.get("mean_full"):
        count = shape[-2] * shape[-1] * (shape[1] if start == 1 else 1)
        return m.flatten(start).sum(-1) / count
    return m.flatten(start).mean(-1)


def ssim(x, y, knobs=None, exact_taps=False):
    knobs = knobs or {}
    ss, _ = ssim_maps(x, y, knobs, exact_taps)
    return _mean(ss, 1, x.shape, knobs)


def _pool(x, knobs):
    if knobs.get("pool_div4"):        # a window hanging over the edge still divides by 4
        return F.avg_pool2d(F.pad(x, (0, x.shape[-1] % 2, 0, x.shape[-2] % 2)), kernel_size=2)
    return F.avg_pool2d(x, kernel_size=2, ceil_mode=True)


def ms_ssim_planes(x, y, knobs=None, exact_taps=False):
    """prod_i relu(cs_i or ss_5)^w_i per (sample, channel): [N, C]"""
    knobs = knobs or {}
    wl = list(MS_WEIGHTS)
    if knobs.get("weights_swapped"):  # the two closest weights: the hardest exchange to see
        wl[1], wl[2] = wl[2], wl[1]
    w = torch.tensor(wl, dtype=x.dtype)
    vals = []
    for i in range(len(MS_WEIGHTS)):
        if i > 0:
            x, y = _pool(x, knobs), _pool(y, knobs)
        ss, cs = ssim_maps(x, y, knobs, exact_taps)
        last = i + 1 == len(MS_WEIGHTS)
        v = _mean(ss if last and not knobs.get("last_cs") else cs, 2, x.shape, knobs)
        vals.append(v if knobs.get("no_relu") else torch.relu(v))
    ms = torch.stack(vals, dim=-1) ** w
    return ms.prod(dim=-1)


def ms_ssim(x, y, knobs=None, exact_taps=False):
    return ms_ssim_planes(x, y, knobs, exact_taps).mean(dim=-1)


def score(mode, x, y, knobs=None, exact_taps=False):
    return (ms_ssim if mode == "msssim" else ssim)(x, y, knobs, exact_taps)


def loss_and_grad(mode, x, y, dtype, knobs=None):
    """scores [N], loss = WEIGHT * mean_n (1 - score_n) and d loss / d x by torch autograd, all in dtype"""
    xr = x.detach().to(dtype, copy=True).requires_grad_()
    s = score(mode, xr, y.to(dtype), knobs)
    loss = WEIGHT * (1 - s).mean()
    loss.backward()
    return s.detach(), loss.detach(), xr.grad


def tap_distance(mode, x, y):
    """|float64 on float64 taps - float64 on the fp32-rounded taps|, worst sample (information only)"""
    xd, yd = x.double(), y.double()
    return (score(mode, xd, yd, exact_taps=True) - score(mode, xd, yd)).abs().max().item()


# ---------------------------------------------------------------------------- regimes

def _smooth(g, c, h, w, cell=8):
    coarse = torch.rand(1, c, max(h // cell, 2), max(w // cell, 2), generator=g)
    return F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[0]


def _texture_target(g, c, h, w):
    return 0.2 + 0.6 * (0.7 * _smooth(g, c, h, w) + 0.3 * _smooth(g, c, h, w, cell=2))


def _noisy(g, t, sigma):
    return (t + sigma * torch.randn(t.shape, generator=g)).clip(0, 1)


def _dark_exposure(g, c, h, w):
    """a low-light frame through an under-trained denoiser: the exposure is off, the means of x and y differ, c1 decides"""
    t = 0.01 + 0.05 * _smooth(g, c, h, w)
    return (0.6 * t + 0.004 * torch.randn(t.shape, generator=g)).clip(0, 1), t


def _bright_flat(g, c, h, w):
    """variance ~1e-5 against means ~0.8: E[xx] - mu^2 cancels seven digits"""
    t = 0.9 + 0.01 * (2 * _smooth(g, c, h, w) - 1)
    return _noisy(g, t, 0.003), t


def _texture(g, c, h, w):
    t = _texture_target(g, c, h, w)
    return _noisy(g, t, 0.03), t


def _near(g, c, h, w):
    """training near convergence: the gradient is a small difference of large terms.  Noise 2e-3: at 1e-3 R32's own corner-side
    class (2,1) of 161 x 161 MS-SSIM is 1.7e-2 from float64, a bar of 0.17 and over CLASS_BAR_CAP; at 2e-3 the widest bar is 3.7e-2"""
    t = _texture_target(g, c, h, w)
    return _noisy(g, t, 2e-3), t


def _identical(g, c, h, w):
    t = _texture_target(g, c, h, w)
    return t.clone(), t


def _dead_plane(g, c, h, w):
    """a correlated pair whose last channel has y = 1 - x: s_xy = -s_xx there, that plane's cs <= 0 and its product is 0"""
    x, t = _texture(g, c, h, w)
    t = t.clone()
    t[-1] = 1 - x[-1]
    return x, t


GENERATORS = {"dark_exposure": _dark_exposure, "bright_flat": _bright_flat, "texture": _texture, "near": _near,
              "identical": _identical, "dead_plane": _dead_plane}
REGIMES = {"ssim": ("dark_exposure", "bright_flat", "texture", "near", "identical"),
           "msssim": ("dark_exposure", "bright_flat", "texture", "near", "identical", "dead_plane")}
SHAPES = {"ssim": ((1, 1, 11, 11),        # one window
                   (2, 3, 42, 43),        # valid map 32 x 33: one column into the second forward tile
                   (1, 3, 17, 75),        # one row into the second backward tile; valid width 65
                   (3, 1, 33, 48),
                   (1, 3, 64, 21)),
          "msssim": ((1, 3, 161, 161),    # 161 -> 81 -> 41 -> 21 -> 11: odd at every level, one position at the top
                     (2, 3, 176, 208),    # even throughout; 208 -> ... -> 13
                     (1, 1, 163, 301),    # mixed parity
                     (1, 3, 177, 162))}


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def sample_regimes(mode, shape, first):
    """the regime of every sample: `first`, then the ones after it in the mode's list, so that a batch mixes regimes"""
    names = REGIMES[mode]
    k = names.index(first)
    return tuple(names[(k + i) % len(names)] for i in range(shape[0]))


def make_pair(mode, shape, first):
    n, c, h, w = shape
    xs, ys = [], []
    for i, name in enumerate(sample_regimes(mode, shape, first)):
        g = torch.Generator().manual_seed(zlib.crc32(f"{mode} {shape_id(shape)} {first} {i} {name}".encode()))
        x, y = GENERATORS[name](g, c, h, w)
        xs.append(x)
        ys.append(y)
    return torch.stack(xs).contiguous(), torch.stack(ys).contiguous()


# ---------------------------------------------------------------------------- edge classes

@functools.lru_cache(maxsize=None)
def class_ids(h, w):
    """[h, w] int64: (min(d_y, 10), min(d_x, 10)) as 11 * that row class + the column class"""
    ry, rx = torch.arange(h), torch.arange(w)
    dy = torch.minimum(ry, h - 1 - ry).clamp(max=REACH)
    dx = torch.minimum(rx, w - 1 - rx).clamp(max=REACH)
    return dy[:, None] * (REACH + 1) + dx[None, :]


def class_name(k):
    return f"({k // (REACH + 1)},{k % (REACH + 1)})"


def class_present(h, w):
    return torch.bincount(class_ids(h, w).flatten(), minlength=NCLASS) > 0


def class_max(t):
    """max |t| per (sample, class) over channels and the class's pixels: [N, 121] float64 (0 where the image has no such pixel;
    NaN where a member is NaN)"""
    n, _, h, w = t.shape
    v = t.detach().double().abs().amax(dim=1).flatten(1)                      # amax propagates NaN
    ids = class_ids(h, w).flatten()[None].expand(n, -1)
    return torch.zeros(n, NCLASS, dtype=torch.float64).scatter_reduce(1, ids, v, "amax", include_self=True)


# ---------------------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def case(mode, shape, first):
    """Inputs, both references and the bars of one case, made once and shared (leave them unchanged)."""
    x, y = make_pair(mode, shape, first)
    s64, l64, g64 = loss_and_grad(mode, x, y, torch.float64)
    s32, l32, g32 = loss_and_grad(mode, x, y, torch.float32)
    score_bar = (FACTOR * (s32.double() - s64).abs()).clamp(min=SCORE_FLOOR)
    return dict(mode=mode, shape=shape, first=first, regimes=sample_regimes(mode, shape, first), x=x, y=y,
                s64=s64, s32=s32, loss64=l64.item(), g64=g64, g32=g32, score_bar=score_bar,
                present=class_present(*shape[2:]), den=class_max(g64), num32=class_max(g32.double() - g64), abs32=class_max(g32))


def case_id(mode, shape, first):
    return f"{mode}-{shape_id(shape)}-{first}"


def all_cases(mode=None):
    return [(m, s, r) for m in (("ssim", "msssim") if mode is None else (mode,)) for s in SHAPES[m] for r in REGIMES[m]]


def grad_report(cs, g):
    """Per sample, a gradient held class by class.  Returns a list of dicts:
      kind  'rel' : fig = max_class |g - g64| / max_class |g64|, bar = 10 x the same figure of R32's autograd gradient
            'abs' : g64 is 0 throughout (x == y, or a sample that is one dead plane): fig = max_class |g|, bar = 10 max_class |g32|
      fig, bar [121] (only `present` classes count), num = max_class |g - g64|, ratio = num / R32's num (GPU / R32, information)"""
    num = class_max(g.double() - cs["g64"])
    out = []
    for i, regime in enumerate(cs["regimes"]):
        den, present = cs["den"][i], cs["present"]
        if regime == "identical" or not den.any():
            assert cs["g64"][i].abs().max() <= 1e-12, (regime, "the float64 gradient of this sample is expected to be 0")
            fig, bar, ref = class_max(g[i:i + 1])[0], FACTOR * cs["abs32"][i], cs["abs32"][i]
            kind, top = "abs", fig
        else:
            assert (den[present] > 0).all(), (regime, "a class without a float64 gradient")
            safe = torch.where(den > 0, den, torch.ones_like(den))
            fig, bar, ref = num[i] / safe, FACTOR * cs["num32"][i] / safe, cs["num32"][i]
            kind, top = "rel", num[i]
        ratio = torch.where(ref > 0, top / torch.where(ref > 0, ref, torch.ones_like(ref)),
                            torch.where(top > 0, torch.full_like(top, float("inf")), torch.zeros_like(top)))
        ratio = torch.where(present, ratio, torch.zeros_like(ratio))
        out.append(dict(sample=i, regime=regime, kind=kind, fig=fig, bar=bar, present=present, ratio=ratio))
    return out


def dead_planes(cs):
    """(sample, channel) of the planes with y = 1 - x"""
    return [(i, cs["shape"][1] - 1) for i, r in enumerate(cs["regimes"]) if r == "dead_plane"]
