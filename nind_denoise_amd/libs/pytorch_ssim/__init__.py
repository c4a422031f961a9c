"""The SSIM the reference vendors in its own tree, on the HIP path.
Interface of the reference's libs/pytorch_ssim/__init__.py:42-68: ``SSIM(window_size=11, size_average=True)`` (an nn.Module) and
``ssim(img1, img2, window_size=11, size_average=True)``.  It is the score behind loss.gen_score / res.txt, not the piqa score of
common/libs/pt_losses.py: the Gaussian window (sigma 1.5) is applied with zero padding of window_size // 2, so the map has
the size of the image and border pixels see zeros; the result is one mean over everything, or one per sample.

The arithmetic runs in ``libnind_hip.so`` (csrc/ssim_padded.hip: nd_ssim_padded, nd_ssim_padded_grad); there is no CPU
fallback.  Inputs are cast to contiguous float32; the call runs on the current stream.  Differentiable with respect to ``img1``;
``img2`` is a constant (the reference would differentiate it too: asking for that raises instead of returning no gradient).
``window_size`` must be odd and within 3...11: an even window makes the reference's map one row and column larger than the image."""
import torch

from ... import _lib

MAX_WINDOW = 11


def _check_window(window_size):
    if not isinstance(window_size, int) or window_size < 3 or window_size > MAX_WINDOW or window_size % 2 == 0:
        raise ValueError(f"window_size must be odd and within 3...{MAX_WINDOW}, got {window_size!r}")
    return window_size


def _prep(img1, img2):
    if img1.shape != img2.shape or img1.dim() != 4:
        raise ValueError(f"expected two [N,C,H,W] tensors of one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.device.type != "cuda" or img2.device != img1.device:
        raise RuntimeError("pytorch_ssim runs on the GPU only (no CPU fallback): move both images to the device")
    return img1.detach().to(torch.float32).contiguous(), img2.detach().to(torch.float32).contiguous()


def _workspace(lib, x, window_size):
    n, c, h, w = x.shape
    return torch.empty(max(lib.nd_ssim_padded_workspace_bytes(n, c, h, w, window_size), 256), dtype=torch.uint8, device=x.device)


class _SsimFn(torch.autograd.Function):
    """Per-sample scores [N]; backward through nd_ssim_padded_grad."""

    @staticmethod
    def forward(ctx, img1, img2, window_size):
        x, y = _prep(img1, img2)
        n, c, h, w = x.shape
        lib = _lib.load()
        ws = _workspace(lib, x, window_size)
        out = torch.empty(n, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.nd_ssim_padded(x.data_ptr(), y.data_ptr(), n, c, h, w, window_size, out.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _lib.stream_ptr(x.device)), "nd_ssim_padded")
        ctx.window_size = window_size
        ctx.save_for_backward(img1, img2)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        img1, img2 = ctx.saved_tensors
        x, y = _prep(img1, img2)
        n, c, h, w = x.shape
        lib = _lib.load()
        ws = _workspace(lib, x, ctx.window_size)
        go = grad_out.detach().to(torch.float32).contiguous()
        gx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.nd_ssim_padded_grad(x.data_ptr(), y.data_ptr(), n, c, h, w, ctx.window_size, go.data_ptr(),
                                               gx.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)),
                       "nd_ssim_padded_grad")
        return gx.to(img1.dtype), None, None


def ssim(img1, img2, window_size=11, size_average=True):
    """0-dim mean of the per-sample scores (size_average) or the scores [N]."""
    _check_window(window_size)
    if img2.requires_grad:
        raise NotImplementedError("pytorch_ssim: the gradient with respect to img2 is not implemented (img2 is a constant here; "
                                  "detach it, or swap the arguments: the score is symmetric)")
    scores = _SsimFn.apply(img1, img2, window_size)
    return scores.mean() if size_average else scores


class SSIM(torch.nn.Module):
    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = _check_window(window_size)
        self.size_average = size_average

    def forward(self, img1, img2):
        return ssim(img1, img2, self.window_size, self.size_average)
