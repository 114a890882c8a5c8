"""CPU: the training-side restatement of the Swin condition encoder (tests/swin_train_ref.py: fp64 autograd over tests/swin_ref.py,
stochastic depth as row scales) against the gradients the reference's own classes gave in float64 and train mode
(tests/golden/g20_swin_train.npz, written by tools/make_golden_swin_train.py), and the bookkeeping of
``SwinTransformer.enable_training()`` and ``Unet(..., train_cond_encoder=True)``."""
import json

import numpy as np
import pytest
import torch

import swin_ref as R
import swin_train_ref as T


@pytest.fixture(scope="module")
def golden():
    return T.load_golden()


def _same(got, want):
    want = np.asarray(want)
    np.testing.assert_allclose(T.sample_grad(got.detach()).numpy(), want, rtol=1e-10, atol=1e-10 * float(np.abs(want).max()))


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_ref_attention_gradients_reproduce_golden(golden, name):
    for k, g in T.attn_module_grads(name).items():
        _same(g, golden[f"attn.{name}.{k}"])


@pytest.mark.parametrize("name", ["a5x5", "a9x10"])
def test_padding_keys_send_their_gradient_to_the_bias(name):
    """The attention core alone: the bias operand is what padding tokens have as key and value, never as query."""
    _, d_qb, _, _ = T.attn_core_grads(name)
    C = d_qb.numel() // 3
    assert float(d_qb[:C].abs().max()) == 0.0
    assert float(d_qb[C:2 * C].abs().max()) > 0.0 and float(d_qb[2 * C:].abs().max()) > 0.0


@pytest.mark.parametrize("name", list(R.MERGE_CASES))
def test_ref_patch_merging_gradients_reproduce_golden(golden, name):
    for k, g in T.merge_grads(name).items():
        _same(g, golden[f"merge.{name}.{k}"])


@pytest.mark.parametrize("tag,p,keep", [("small.sd0", 0.0, None), ("small.sd5", 0.5, T.KEEP_SMALL)])
def test_ref_model_gradients_reproduce_golden(golden, tag, p, keep):
    grads = T.model_grads(R.SMALL, R.SMALL_INPUT, "small", tag, keep, p)
    assert list(grads) == json.loads(str(golden[f"{tag}.names"])) and len(grads) == 118
    for k, g in grads.items():
        _same(g, golden[f"{tag}.{k}"])


def test_injected_draws_drop_a_sample_in_a_late_block():
    probs = T.sd_probs(R.SMALL["depths"], 0.5)
    assert probs[0] == 0.0 and probs[-1] == 0.5
    assert float(T.KEEP_SMALL[-1].min()) == 0.0 and float(T.KEEP_SMALL[1:].sum(dim=(0, 1)).min()) > 0
    scales = T.scales_from_keep(T.KEEP_SMALL, probs)
    assert scales[0] is None and scales[-1].tolist() == [[0.0, 2.0], [2.0, 2.0]]


# ------------------------------------------------------------------------------------------------ enable_training() bookkeeping
def _small(**kw):
    from adm_amd.unet.swin_transformer import SwinTransformer
    return SwinTransformer(patch_size=[4, 4], embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=[7, 7], **kw)


def test_default_construction_is_unchanged():
    from adm_amd.unet.swin_transformer import swin_b
    for m in (_small(), _small(stochastic_depth_prob=0.5), swin_b()):
        assert not m.trainable and all(not p.requires_grad for p in m.parameters())
        assert all(b.sd_prob == 0.0 for b in m.blocks())
    with pytest.raises(RuntimeError, match="enable_training"):
        _small()(torch.zeros(1, 3, 32, 32), keep=torch.ones(8, 2, 1))


def test_enable_training_marks_what_forward_uses():
    m = _small()
    assert m.enable_training() is m and m.trainable
    sd = R.filled_state_dict(**R.SMALL)
    want = set(T.trainable_names(sd))
    got = {k for k, p in m.named_parameters() if p.requires_grad}
    assert got == want and len(got) == 117
    frozen = {k for k, p in m.named_parameters() if not p.requires_grad}
    assert frozen == {"norm.weight", "norm.bias", "head.weight", "head.bias"}
    assert all(b.sd_prob == 0.0 for b in m.blocks())          # the constructor's stochastic_depth_prob (0.0)
    # the state_dict is what it was
    assert [k for k in m.state_dict()] == list(sd)


def test_stochastic_depth_schedule():
    from adm_amd.unet.swin_transformer import swin_b
    m = swin_b()
    assert m.stochastic_depth_prob == 0.5
    m.enable_training()
    ps = [b.sd_prob for b in m.blocks()]
    assert len(ps) == 24 and ps[0] == 0.0 and ps[-1] == 0.5
    assert ps == pytest.approx([0.5 * k / 23 for k in range(24)], abs=1e-15) and ps == T.sd_probs(R.SWIN_B["depths"], 0.5)
    m.enable_training(0.0)
    assert all(b.sd_prob == 0.0 for b in m.blocks())
    m.enable_training(0.2)
    assert m.blocks()[-1].sd_prob == pytest.approx(0.2) and m.stochastic_depth_prob == 0.5
    with pytest.raises(ValueError):
        m.enable_training(1.0)
    keep = m.draw_keep(3, torch.device("cpu"))
    assert tuple(keep.shape) == (24, 2, 3) and bool(keep[0].all()) and set(keep.unique().tolist()) <= {0.0, 1.0}


def _unet(U, **kw):
    return U.Unet(dim=32, dim_mults=(1, 2, 4, 8), cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=3,
                  window_sizes1=[[8, 8], [4, 4], [2, 2], [1, 1]], window_sizes2=[[8, 8], [4, 4], [2, 2], [1, 1]], fourier_scale=16,
                  cfg={"cond_net": "swin"}, **kw)


def test_unet_train_cond_encoder_wiring():
    import adm_amd.unet.cond_unet as U2
    import adm_amd.unet.cond_unet_sd as U1
    for U in (U1, U2):
        m = _unet(U, cond_encoder="swin_b", train_cond_encoder=True)
        enc = m.init_conv_mask
        assert enc.trainable and enc.blocks()[-1].sd_prob == 0.5
        on = {k for k, p in enc.named_parameters() if p.requires_grad}
        assert "first_coonv.0.weight" in on and "features.6.1.mlp.3.bias" in on and not any(k.startswith(("norm.", "head.")) for k in on)
        with pytest.raises(ValueError, match="fix_bb"):
            _unet(U, cond_encoder="swin_b", train_cond_encoder=True, fix_bb=True)
        with pytest.raises(ValueError, match="swin_b"):
            _unet(U, train_cond_encoder=True)
        frozen = _unet(U, cond_encoder="swin_b")          # the default stays frozen
        assert not frozen.init_conv_mask.trainable and all(not p.requires_grad for p in frozen.init_conv_mask.parameters())
