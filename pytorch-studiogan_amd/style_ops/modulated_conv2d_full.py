"""StyleGAN3's modulated convolution (reference src/models/stylegan3.py:24-63) on the kernel of modulated_conv2d.py. It differs from StyleGAN2's in three ways:

  * weight and styles are pre-normalised when demodulating: W / rms(W) per output channel, s / rms(s) over the whole [N, I] batch. Both are small plain-torch
    expressions in front of the kernel, differentiated by autograd; the demodulation d = (sum (W s)^2 + 1e-8)^(-1/2) is then the kernel's own;
  * full padding, k - 1 per side (output H + k - 1). The kernel (sg_modconv2d_ok) serves stride 1 at pad k / 2 only, and taking the full-padding descriptor
    needs kernel work, so x is zero-padded by (k - 1) / 2 per side in front of the `same` mode: the same arithmetic, one small copy of x for k = 3,
    none for k = 1. The data gradient is the same-mode gradient cropped by autograd;
  * a scalar input_gain behind the demodulation (magnitude_ema.rsqrt(), a constant): folded into the per-[N, Cout] post-scale table (_ModConvFn's
    post_gain), with demodulate=False (ToRGB) the table is that gain alone. No elementwise pass of its own.
First-order gradients only, like modulated_conv2d."""
import torch
import torch.nn.functional as F

from .. import _lib as L
from .modulated_conv2d import _ModConvFn, _validate_kernel, _validate_operands


def modulated_conv2d(x, w, s, demodulate=True, padding=0, input_gain=None):
    """The reference's signature. x: [N, I, H, W] float32 or bfloat16; w: [O, I, k, k], k = 1 or 3; s: [N, I]; padding: k - 1; input_gain: None or a scalar
    tensor (a per-channel or per-sample gain is refused: the networks pass magnitude_ema.rsqrt()). The result is channels_last."""
    k = _validate_kernel("modulated_conv2d (full)", *_validate_operands("modulated_conv2d (full)", x, w, s)[-2:])
    if padding != k - 1:
        raise NotImplementedError(f"modulated_conv2d (full): padding={padding} is not supported (padding = kernel_size - 1 = {k - 1})")
    if input_gain is not None and not (isinstance(input_gain, torch.Tensor) and input_gain.numel() == 1):
        raise NotImplementedError("modulated_conv2d (full): input_gain must be a scalar tensor")
    L.require_gpu(x.device)
    if demodulate:
        w = w * w.square().mean([1, 2, 3], keepdim=True).rsqrt()
        s = s * s.square().mean().rsqrt()
    if k == 3:
        x = F.pad(x, [1, 1, 1, 1])
    return _ModConvFn.apply(x, w, s, None, 1, bool(demodulate), True, input_gain)
