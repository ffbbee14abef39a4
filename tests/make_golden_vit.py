"""Writes tests/golden/vit_small.npz: input, `embed` and `logits` of the REAL reference VisionTransformer (src/metrics/vit.py, loaded by file path)
on the seeded small geometry of tests/vit_ref.py, after asserting that the restatement there reproduces the reference bit for bit in fp32.
Weights are not stored: the tests regenerate them from the seed.

    python tests/make_golden_vit.py /path/to/StudioGAN [--check]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vit_ref as VR  # noqa: E402

SEED, INPUT_SEED, BATCH = 11, 1, 3
FIXTURE = os.path.join(HERE, "golden", "vit_small.npz")


def load_reference_vit(reference_root):
    path = os.path.join(reference_root, "src", "metrics", "vit.py")
    spec = importlib.util.spec_from_file_location("reference_vit", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_outputs(reference_root, geo=VR.SMALL):
    """(x, embed, logits) of the reference module with the seeded weights; asserts the restatement is bit-identical."""
    vits = load_reference_vit(reference_root)
    torch.manual_seed(0)
    from functools import partial
    model = vits.VisionTransformer(img_size=[geo["img"]], patch_size=geo["patch"], num_classes=geo["classes"], embed_dim=geo["embed"], depth=geo["depth"],
                                   num_heads=geo["heads"], mlp_ratio=4, qkv_bias=True, num_last_blocks=geo["num_last_blocks"],
                                   norm_layer=partial(torch.nn.LayerNorm, eps=VR.LN_EPS))
    sd = VR.random_state_dict(SEED, geo)
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = VR.small_input(INPUT_SEED, BATCH, geo)
    with torch.no_grad():
        embed, logits = model(x)
        e2, l2 = VR.vit_forward(sd, x, geo["heads"], geo["num_last_blocks"])
    assert torch.equal(embed, e2) and torch.equal(logits, l2), "tests/vit_ref.py does not reproduce the reference bit for bit"
    return x, embed, logits


def main():
    root = sys.argv[1]
    x, embed, logits = reference_outputs(root)
    if "--check" in sys.argv:
        z = np.load(FIXTURE)
        assert np.array_equal(z["x"], x.numpy()) and np.array_equal(z["embed"], embed.numpy()) and np.array_equal(z["logits"], logits.numpy())
        print("fixture matches the reference")
        return
    np.savez_compressed(FIXTURE, x=x.numpy(), embed=embed.numpy(), logits=logits.numpy())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
