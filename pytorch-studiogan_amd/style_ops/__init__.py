"""Host mirrors of the reference's StyleGAN2 / StyleGAN3 native operators (reference src/utils/style_ops/{bias_act,upfirdn2d,filtered_lrelu}.py,
SURVEY.md 8(f4)): same function names, argument meaning and error behaviour, every launch a kernel of libsgamd.so (csrc/style.hip).
`impl='cuda'` (the default, kept for call-site compatibility -- on PyTorch-ROCm the device type is still 'cuda') runs the HIP kernels;
there is no `impl='ref'` here: the reference path lives in the reference and, restated for the tests, in oracle/style_ref.py.
modulated_conv2d (reference src/models/stylegan2.py:28-98, the operator StyleGAN2's synthesis layers are made of) runs on csrc/modconv.hip, and so does
modulated_conv2d_full (StyleGAN3's variant, src/models/stylegan3.py:24-63: pre-normalised, full padding, input_gain);
fir_bias_act (no counterpart in the reference: the FIR + noise + bias + activation tail of an up = 2 synthesis layer in one launch) on csrc/style_fir.hip."""
from . import bias_act, upfirdn2d, filtered_lrelu, modulated_conv2d, modulated_conv2d_full, fir_bias_act  # noqa: F401
from ..functional._base import second_order  # noqa: F401      (the opt-in of the discriminator operators' differentiable backward: R1)
