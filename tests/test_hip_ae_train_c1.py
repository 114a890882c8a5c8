"""GPU parity tests of the ONE-channel KL autoencoder's training path (AutoencoderKL(in_channels=1, out_ch=1) with
LPIPSWithDiscriminator(disc_in_channels=1): the first stage of the latent saliency recipe): the NLL term and the PatchGAN
discriminator at one channel against fp64 torch as tests/test_hip_ae_train.py checks them at three, and both training steps
against the reference's fp64 results (tests/golden/g27_ae_train_c1.npz, written by tools/make_golden_ae_train_c1.py) at 64x48 --
non-square, so that an H / W mix-up in a one-channel layout kernel shows."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import fill

import ae_train_c1_ref as R1
import ae_train_ref as R
import lpips_ref
from parity import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def nhwc(x, cpad):
    B, C, H, W = x.shape
    y = torch.zeros(B, H, W, cpad, dtype=x.dtype)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y


def rel_l2(got, want):
    got, want = got.detach().cpu().double().reshape(-1), torch.as_tensor(np.asarray(want)).double().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


@pytest.mark.parametrize("shape", [(2, 1, 16, 16), (3, 1, 5, 7)])
def test_nll_one_channel_vs_torch(gpu, shape):
    """nll_loss and rec_loss with the [B,1,1,1] LPIPS value broadcast over every element of a ONE-channel image, and the gradients
    to the reconstruction, the LPIPS values and logvar.  (3, 1, 5, 7): 105 elements, no multiple of four."""
    from adm_amd import ops_ae
    B = shape[0]
    x, r = fill.hash_tensor(shape, "nll1.x", 1.0), fill.hash_tensor(shape, "nll1.r", 1.0)
    p = fill.hash_tensor((B,), "nll1.p", 0.3).abs()
    lv = torch.tensor(0.37)
    rd, lvd, pd = r.double().requires_grad_(), lv.double().requires_grad_(), p.double().requires_grad_()
    rec = (x.double() - rd).abs() + (x.double() - rd) ** 2 + 0.8 * pd.reshape(B, 1, 1, 1)
    nll = torch.sum(rec / torch.exp(lvd) + lvd) / B
    (1.7 * nll).backward()
    rg, lvg, pg = r.to(gpu).requires_grad_(), lv.to(gpu).requires_grad_(), p.to(gpu).requires_grad_()
    out = ops_ae.nll_terms(x.to(gpu), rg, pg, lvg, 0.8)
    close(out[0], nll)
    close(out[1], rec.mean())
    (1.7 * out[0]).backward()
    close(rg.grad, rd.grad)
    close(lvg.grad, lvd.grad)
    close(pg.grad, pd.grad)


def _torch_discriminator(sd, input_nc):
    """The reference's nn.Sequential, rebuilt: 4x4 convs, BatchNorm2d, LeakyReLU(0.2)."""
    seq = []
    layers = R.disc_layers(input_nc)
    for i, ci, co, stride, bias, bn in layers:
        seq.append(nn.Conv2d(ci, co, 4, stride, 1, bias=bias))
        if bn:
            seq.append(nn.BatchNorm2d(co))
        if i != layers[-1][0]:
            seq.append(nn.LeakyReLU(0.2, True))
    m = nn.Module()
    m.main = nn.Sequential(*seq)
    m.load_state_dict(sd, strict=True)
    return m.double()


@pytest.mark.parametrize("training", [True, False])
def test_discriminator_one_channel_vs_torch(gpu, training):
    """input_nc = 1: logits, the gradient at the input (one real channel, 31 pad channels that must stay zero), every parameter
    gradient and the BatchNorm running statistics against fp64 torch; 48x40 input (odd map sizes after the stride-1 convs)."""
    from adm_amd.ddm.loss import NLayerDiscriminator
    sd = R.disc_state(3.0, input_nc=1, tag="disc.c1")
    x = fill.hash_tensor((2, 1, 48, 40), "disc1.x", 1.0)
    ref = _torch_discriminator(sd, 1).train(training)
    xd = x.double().requires_grad_()
    want = ref.main(xd)
    dy = fill.hash_tensor(tuple(want.shape), "disc1.dy", 1.0)
    want.backward(dy.double())
    D = NLayerDiscriminator(input_nc=1).to(gpu).train(training)
    D.load_state_dict(sd, strict=True)
    assert tuple(D.main[0].weight.shape) == (64, 1, 4, 4)
    xg = nhwc(x, 32).to(gpu).requires_grad_()
    y = D(xg)
    assert y.shape == (2, want.shape[2], want.shape[3], 32)
    close(y[..., :1].permute(0, 3, 1, 2), want)
    assert float(y.detach()[..., 1:].abs().max()) == 0.0
    y.backward(nhwc(dy, 32).to(gpu))
    close(xg.grad[..., :1].permute(0, 3, 1, 2), xd.grad)
    rp = dict(ref.named_parameters())
    for k, p in D.named_parameters():
        assert p.grad.shape == rp[k].grad.shape, k
        e = rel_l2(p.grad, rp[k].grad)
        print(f"training={training} grad {k}: rel L2 {e:.2e}")
        assert e < 2e-3, k
        close(p.grad, rp[k].grad)
    rs = ref.state_dict()
    for k, v in D.state_dict().items():
        if "running" in k or "num_batches" in k:
            close(v, rs[k], rtol=1e-5, atol=1e-6)
            assert torch.equal(v.cpu().double(), sd[k].double()) == (not training), k        # untouched in eval()


# ------------------------------------------------------------------------------------------------ training steps vs golden
DD = dict(double_z=True, z_channels=3, resolution=list(R1.RES), in_channels=1, out_ch=1, ch=R1.CH, ch_mult=[1, 2, 4], num_res_blocks=2,
          attn_resolutions=[], dropout=0.0)
D_WEIGHT_BAR = 1e-3          # max(1e-3, 4 x 7.0e-7): tests/test_image_data_host.py measures fp32 torch's deviation


def build_trainable(gpu, tag):
    import importlib
    from adm_amd.ddm.lpips import LPIPS
    ED = importlib.import_module("ddm.encoder_decoder")
    ae = ED.AutoencoderKL(DD, dict(R1.LOSSCONFIG), 3)
    ae.enable_training(lpips=LPIPS.from_state_dict(lpips_ref.synthetic_state_dict()))
    assert ae.encoder.conv_in.weight.shape[1] == 1 and ae.decoder.conv_out.weight.shape[0] == 1
    assert ae.loss.discriminator.main[0].weight.shape[1] == 1
    msg = ae.load_state_dict(R1.case_state(tag, torch.float32), strict=False)
    assert not msg.unexpected_keys and all(k.startswith("loss.perceptual_loss.") for k in msg.missing_keys)
    return ae.to(gpu).train()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "g27_ae_train_c1.npz"))


@pytest.mark.parametrize("tag,idx", R1.CASES)
def test_train_step_one_channel_vs_golden(gpu, gold, tag, idx):
    """One training micro-step of the one-channel autoencoder against the reference's fp64 results, with the bars of
    tests/test_hip_ae_train.py test_train_step_vs_golden: log values at rtol 1e-3, gradients at 2e-3 relative L2, d_weight at
    max(1e-3, 4 x the fp32-torch deviation) = 1e-3 (the host test measures that deviation as 7.0e-7 'pre' and 1.5e-7 'post').
    Measured on an MI355X: d_weight 1.5e-6 ('pre') / 4.2e-5 ('post') off, logs <= 1.0e-6, gradients <= 2.3e-5 ('pre') and
    5.4e-4 .. 1.5e-3 ('post') relative L2.  The 'post' figures are one flipped kink element, not the channel count or the shape:
    on other fills of the same one-channel 64x48 model the same step lands 4e-5 from fp64, and there fp32 torch is the one that
    flips (1e-2 on a three-channel fill).
    The step must leave the other optimiser's gradients untouched, and update the BatchNorm statistics once (generator step) or
    twice (discriminator step: real, then fake)."""
    ae = build_trainable(gpu, tag)
    x, eps = R1.case_inputs(tag)
    loss, log = ae.training_step(x.to(gpu), idx, R1.STEPS[tag], eps=eps.to(gpu))
    key = f"{tag}.opt{idx}"
    checks = []
    for k in gold.files:
        if k.startswith(f"{key}.log."):
            name = k[len(key) + 5:]
            got, want = float(log[name]), float(gold[k])
            print(f"{key} {name}: {got:.8g} (golden {want:.8g}), off {abs(got - want) / max(abs(want), 1e-30):.2e}")
            bar = D_WEIGHT_BAR if name.endswith("d_weight") else 1e-3
            checks.append((abs(got - want) <= bar * abs(want) + 1e-7, (name, got, want)))
            assert isinstance(log[name], torch.Tensor)
    params = dict(ae.named_parameters())
    n = 0
    for k in gold.files:
        if k.startswith(f"{key}.grad."):
            name = k[len(key) + 6:]
            assert tuple(params[name].grad.shape) == tuple(gold[k].shape), name
            e = rel_l2(params[name].grad, gold[k])
            print(f"{key} grad {name}: rel L2 {e:.2e}")
            checks.append((e < 2e-3, (name, e)))
            n += 1
    assert n == len(R1.grad_keys(tag, idx))
    for ok, what in checks:          # every figure is printed before the first assertion
        assert ok, what
    assert abs(float(loss) - float(gold[f"{key}.loss"])) <= 1e-3 * abs(float(gold[f"{key}.loss"])) + 1e-7
    for name, p in params.items():
        mine = name.startswith("loss.discriminator.") if idx == 1 else not name.startswith("loss.")
        if name.startswith("loss.perceptual_loss."):
            assert p.grad is None, name
        elif name == "loss.logvar":
            assert (p.grad is not None) == (idx == 0)
        else:
            assert (p.grad is not None) == mine, name
    sd = ae.state_dict()
    assert int(sd["loss.discriminator.main.3.num_batches_tracked"]) == int(gold[f"{key}.bn.num_batches_tracked"]) == (1 if idx == 0 else 2)
    for s in ("running_mean", "running_var"):
        close(sd[f"loss.discriminator.main.3.{s}"], gold[f"{key}.bn.{s}"], rtol=1e-4, atol=1e-5)
