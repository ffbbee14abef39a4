"""CPU-side checks of the DINO ViT backbone: the restatement the GPU tests use as oracle against the committed reference outputs, state-dict
validation, the two weight-file layouts, and the backbones that stay out."""
import os

import numpy as np
import pytest
import torch

import vit_ref as VR
import make_golden_vit as MG

REFERENCE = "/root/reference"


def _fixture():
    z = np.load(MG.FIXTURE)
    return torch.from_numpy(z["x"]), torch.from_numpy(z["embed"]), torch.from_numpy(z["logits"])


def test_restatement_matches_reference_fixture():
    x, embed, logits = _fixture()
    assert torch.equal(x, VR.small_input(MG.INPUT_SEED, MG.BATCH))
    sd = VR.random_state_dict(MG.SEED, VR.SMALL)
    e, l = VR.vit_forward(sd, x, VR.SMALL["heads"], VR.SMALL["num_last_blocks"])
    assert e.shape == (MG.BATCH, 4 * VR.SMALL["embed"]) and l.shape == (MG.BATCH, VR.SMALL["classes"])
    assert float((e - embed).abs().max()) <= 1e-5 * float(embed.abs().max())
    assert float((l - logits).abs().max()) <= 1e-5 * float(logits.abs().max())
    e64, l64 = VR.vit_forward_f64(sd, x, VR.SMALL["heads"])
    assert e64.dtype == torch.float64 and float((e64.float() - embed).abs().max()) <= 1e-4 * float(embed.abs().max())


def test_seeded_weights_exercise_attention():
    """the softmax rows of the seeded weights are far from uniform: the largest probability of a row is well above 1 / N"""
    sd = VR.random_state_dict(MG.SEED, VR.SMALL)
    C, heads = VR.SMALL["embed"], VR.SMALL["heads"]
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, 17, C, generator=g)
    qkv = torch.nn.functional.linear(y, sd["blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.bias"]).reshape(2, 17, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (qkv[0] @ qkv[1].transpose(-2, -1)) / 8.0
    assert float(s.std()) > 1.5 and float(s.softmax(-1).max(-1).values.mean()) > 3.0 / 17


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "metrics")), reason="the reference checkout is not on this machine")
def test_fixture_regenerates_from_reference():
    x, embed, logits = MG.reference_outputs(REFERENCE)
    fx, fe, fl = _fixture()
    assert torch.equal(x, fx)
    assert float((embed - fe).abs().max()) <= 1e-5 * float(fe.abs().max()) and float((logits - fl).abs().max()) <= 1e-5 * float(fl.abs().max())


def test_validate_dino_state_dict():
    from studiogan_amd import metrics as M
    sd = VR.random_state_dict(3, VR.SMALL)
    geo = M.validate_dino_state_dict(sd)
    assert (geo["embed"], geo["depth"], geo["heads"], geo["patch"], geo["tokens"], geo["classes"], geo["hidden"]) == (128, 5, 2, 8, 17, 10, 512)
    full = M.dino_manifest(384, 12, 8, 785, 1000)
    assert len(full) == 8 + 12 * 12 and full["blocks.11.mlp.fc1.weight"] == (1536, 384) and full["linear.weight"] == (1000, 1536)
    missing = {k: v for k, v in sd.items() if k != "blocks.2.attn.proj.bias"}
    with pytest.raises(RuntimeError, match="missing 1: blocks.2.attn.proj.bias"):
        M.validate_dino_state_dict(missing)
    wrong = dict(sd)
    wrong["blocks.1.mlp.fc2.weight"] = torch.zeros(128, 256)
    with pytest.raises(RuntimeError, match="wrong shape / dtype 1: blocks.1.mlp.fc2.weight"):
        M.validate_dino_state_dict(wrong)
    extra = dict(sd)
    extra["head.mlp.0.weight"] = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="unexpected 1: head.mlp.0.weight"):
        M.validate_dino_state_dict(extra)
    with pytest.raises(RuntimeError, match="head dimension must be 64"):
        M.validate_dino_state_dict(sd, num_heads=4)                         # 128 / 4 = 32
    with pytest.raises(RuntimeError, match="head dimension must be 64"):
        M.validate_dino_state_dict(VR.random_state_dict(3, dict(VR.SMALL, embed=96)))


def test_weight_file_layouts(tmp_path):
    """src/utils/misc.py:632-691: backbone optionally under "teacher" with module. / backbone. prefixes (and a projection head the model does not
    own), classifier under "state_dict" with module.linear.; a missing path raises with the file names; pinned only under the published names."""
    from studiogan_amd import metrics as M
    sd = VR.random_state_dict(4, VR.SMALL)
    bb = {k: v for k, v in sd.items() if not k.startswith("linear.")}
    lin = {"module.linear.weight": sd["linear.weight"], "module.linear.bias": sd["linear.bias"]}
    plain, lin_path = str(tmp_path / M.DINO_BACKBONE_FILE), str(tmp_path / M.DINO_LINEAR_FILE)
    torch.save(bb, plain)
    torch.save({"state_dict": lin, "epoch": 100}, lin_path)
    got, digests, pinned = M.load_dino_weights(plain, lin_path)
    assert len(digests) == 2 and all(len(d) == 64 for d in digests)
    assert not pinned, "the published names over another geometry (here 128 channels, 5 blocks) must not count as the published weights"
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    ckpt = str(tmp_path / "checkpoint.pth")
    teacher = {"module.backbone." + k: v for k, v in bb.items()}
    teacher["module.head.mlp.0.weight"] = torch.zeros(8, 8)
    torch.save({"teacher": teacher, "student": {}, "epoch": 3}, ckpt)
    got, _, pinned = M.load_dino_weights(ckpt, lin_path)
    assert not pinned and set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match=M.DINO_LINEAR_FILE):
        M.load_dino_weights(plain, str(tmp_path / "nowhere.pth"))
    # pinned needs the published names AND exactly the ViT-S/8 manifest (zero-filled tensors of the right shapes stand in for the files)
    full = {k: torch.zeros(shape) for k, shape in M.dino_manifest(*M.DINO_PUBLISHED_GEOMETRY).items()}
    sub = tmp_path / "published"
    sub.mkdir()
    torch.save({k: v for k, v in full.items() if not k.startswith("linear.")}, str(sub / M.DINO_BACKBONE_FILE))
    torch.save({"state_dict": {"module.linear.weight": full["linear.weight"], "module.linear.bias": full["linear.bias"]}}, str(sub / M.DINO_LINEAR_FILE))
    assert M.load_dino_weights(str(sub / M.DINO_BACKBONE_FILE), str(sub / M.DINO_LINEAR_FILE))[2]
    torch.save({k: v for k, v in full.items() if not k.startswith("linear.")}, str(sub / "renamed.pth"))
    assert not M.load_dino_weights(str(sub / "renamed.pth"), str(sub / M.DINO_LINEAR_FILE))[2]
    with pytest.raises(RuntimeError, match=M.DINO_BACKBONE_FILE):
        M.LoadEvalModel("DINO_torch", "legacy", device="cpu")
    with pytest.raises(RuntimeError, match=M.DINO_BACKBONE_FILE):
        M.LoadEvalModel("DINO_torch", "clean", device="cpu", linear_weights_path=lin_path)


def test_other_backbones_still_raise():
    from studiogan_amd import metrics as M
    for name in ("Swin-T_torch", "SwAV_torch", "ResNet50_torch", "InceptionV3_torch"):
        with pytest.raises(NotImplementedError, match="DINO_torch"):
            M.LoadEvalModel(name, "legacy", device="cpu", state_dict={})
    with pytest.raises(NotImplementedError):
        M.LoadEvalModel("DINO_torch", "nearest", device="cpu", state_dict={})


def test_new_entry_points_are_bound():
    from studiogan_amd import _lib as L
    for name in ("sg_layernorm_rows", "sg_tok_gemm", "sg_mha_fwd", "sg_mha_fwd_ok", "sg_vit_tokens", "sg_gelu_f32", "sg_tok_gemm_launches", "sg_mha_launches",
                 "sg_quantize_resize_normalize_ms", "sg_pil_resize_normalize_ms"):
        assert name in L.exported_symbols()
    lib = L.lib()
    assert lib.sg_mha_fwd_ok(8, 785, 6, 64) == 1 and lib.sg_mha_fwd_ok(8, 785, 6, 32) == 0 and lib.sg_mha_fwd_ok(1, 1, 1, 64) == 1
    assert lib.sg_tok_gemm_launches() >= 0 and lib.sg_mha_launches() >= 0
