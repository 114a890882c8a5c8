"""CPU: the Swin condition encoder's restatement (tests/swin_ref.py) against the float64 outputs the reference's own classes gave
(tests/golden/g19_swin.npz, written by tools/make_golden_swin.py), the module tree's state_dict names / shapes against the
reference's, and the wiring of ``cond_encoder="swin_b"`` into the conditional denoiser."""
import json

import numpy as np
import pytest
import torch

import swin_ref as R


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _same(got, want):
    np.testing.assert_allclose(R.sample(got).numpy(), want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_ref_attention_reproduces_golden(golden, name):
    _same(R.attn_core(*R.attn_case_core(name)), golden[f"attn.{name}"])


@pytest.mark.parametrize("name", list(R.MERGE_CASES))
def test_ref_patch_merging_reproduces_golden(golden, name):
    x, sd = R.merge_case_inputs(name)
    _same(R.merge_ln(x, sd[name + ".norm.weight"], sd[name + ".norm.bias"]), golden[f"merge.{name}.ln"])
    _same(R.patch_merging(sd, name + ".", x), golden[f"merge.{name}.out"])


@pytest.mark.parametrize("name,cfg,shape", [("small", R.SMALL, R.SMALL_INPUT)]
                         + [(n, R.SWIN_B, s) for n, s in R.SWIN_B_INPUTS.items()])
def test_ref_model_reproduces_golden(golden, name, cfg, shape):
    sd = R.filled_state_dict(**cfg)
    ys = R.forward(sd, R.model_input(name, shape), cfg["depths"], cfg["num_heads"])
    assert [list(y.shape) for y in ys] == golden[f"{name}.shapes"].tolist()
    for i, y in enumerate(ys):
        np.testing.assert_allclose(R.sample(y).numpy(), golden[f"{name}.stage{i}"], rtol=1e-12, atol=1e-13)


def test_small_model_output_shapes(golden):
    assert golden["small.shapes"].tolist() == [[2, 32, 18, 22], [2, 64, 9, 11], [2, 128, 5, 6], [2, 256, 3, 3]]


def test_module_state_dict_matches_the_reference(golden):
    from adm_amd.unet.swin_transformer import SwinTransformer, swin_b
    small = SwinTransformer(patch_size=[4, 4], embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=[7, 7])
    for tag, m in (("small", small), ("swin_b", swin_b())):
        want = json.loads(str(golden[f"{tag}.keys"]))
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == want, [a for a, b in zip(got, want) if a != b][:5]
        assert all(not p.requires_grad for p in m.parameters())
        idx = m.state_dict()["features.0.1.attn.relative_position_index"]
        assert torch.equal(idx, R.relative_position_index())
    assert len(json.loads(str(golden["small.keys"]))) == 129
    # a strict load of hash-filled reference-format tensors passes; another index buffer is refused
    sd = R.cast(R.filled_state_dict(**R.SMALL), torch.float32)
    small.load_state_dict(sd, strict=True)
    sd["features.2.1.attn.relative_position_index"] = sd["features.2.1.attn.relative_position_index"].flip(0)
    with pytest.raises(RuntimeError, match="relative_position_index"):
        small.load_state_dict(sd, strict=True)


def test_import_alias():
    import unet.swin_transformer as A
    import adm_amd.unet.swin_transformer as B
    assert A.swin_b is B.swin_b and A.SwinTransformer is B.SwinTransformer
    with pytest.raises(TypeError):
        A.swin_b(weights=None)          # nothing is ever fetched: there is no such argument


def _unet(U, **kw):
    return U.Unet(dim=32, dim_mults=(1, 2, 4, 8), cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=3,
                  window_sizes1=[[8, 8], [4, 4], [2, 2], [1, 1]], window_sizes2=[[8, 8], [4, 4], [2, 2], [1, 1]], fourier_scale=16,
                  cfg={"cond_net": "swin"}, **kw)


def test_unet_wiring(tmp_path):
    import adm_amd.unet.cond_unet as U2
    import adm_amd.unet.cond_unet_sd as U1
    from adm_amd.unet.swin_transformer import SwinTransformer
    plain = _unet(U1)
    assert plain.init_conv_mask is None and not any(k.startswith("init_conv_mask.") for k in plain.state_dict())
    with pytest.raises(NotImplementedError):
        _unet(U1, cond_encoder="swin_b", single_channel_cond=True)
    with pytest.raises(NotImplementedError):
        _unet(U1, cond_encoder="resnet101")
    for U in (U1, U2):
        m = _unet(U, cond_encoder="swin_b", fix_bb=True)
        assert isinstance(m.init_conv_mask, SwinTransformer)
        enc_keys = [k for k in m.state_dict() if k.startswith("init_conv_mask.")]
        assert len(enc_keys) == len(m.init_conv_mask.state_dict()) and "init_conv_mask.first_coonv.0.weight" in enc_keys
        assert all(not p.requires_grad for p in m.init_conv_mask.parameters())
    # init_from_ckpt: a reference-format checkpoint with init_conv_mask.* loads them when the module is there (none missing, none
    # unexpected), and drops them as before when it is not
    m = _unet(U1, cond_encoder="swin_b")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for k in ("init_conv_mask.first_coonv.0.bias", "init_conv_mask.features.6.1.mlp.3.bias", "final_conv.bias"):
        sd[k] = torch.full_like(sd[k], 0.625)
    path = str(tmp_path / "ref.pt")
    torch.save({"model": sd}, path)
    fresh = _unet(U1, cond_encoder="swin_b")
    msg = fresh.load_state_dict(torch.load(path, weights_only=True)["model"], strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    fresh = _unet(U1, cond_encoder="swin_b", ckpt_path=path)
    assert float(fresh.init_conv_mask.first_coonv[0].bias[0]) == 0.625
    assert float(fresh.init_conv_mask.features[6][1].mlp[3].bias[-1]) == 0.625
    plain = _unet(U1, ckpt_path=path)
    assert plain.init_conv_mask is None and float(plain.final_conv.bias[0].detach()) == 0.625
    called = _unet(U1, cond_encoder=lambda c: None, ckpt_path=path)          # a callable: the keys are dropped as before
    assert float(called.final_conv.bias[0].detach()) == 0.625


def test_frozen_backbone_warning():
    from adm_amd.unet.swin_transformer import SwinTransformer
    m = SwinTransformer(patch_size=[4, 4], embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=[7, 7], fix_bb=False)
    m.train()
    with pytest.warns(UserWarning, match="frozen in this build"):
        with pytest.raises(RuntimeError):          # a CPU tensor: the warning comes first, then the HIP path refuses the device
            m(torch.zeros(1, 3, 32, 32))
