"""GPU parity tests of the KL autoencoder's TRAINING path: every new operator (adm_amd/ops_ae.py, csrc/ae_train.hip) forward and
backward against fp64 torch at tests/parity.close (rtol 1e-3, atol 1e-4 x scale), the PatchGAN discriminator against an
nn.Sequential rebuilt here, both training steps against the reference's fp64 results (tests/golden/g18_ae_train.npz, written by
tools/make_golden_ae_train.py), determinism under ADM_DETERMINISTIC=1 and the train_vae.py driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ae_ref, fill

import ae_train_ref as R
import lpips_ref
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("B,H,W,ci,co", [(2, 16, 16, 32, 32), (1, 32, 16, 64, 96), (3, 8, 8, 128, 64), (1, 6, 10, 32, 32)])
def test_conv2d_down_vs_torch(gpu, B, H, W, ci, co):
    """The differentiable Downsample conv at the shapes of test_hip_latent.test_strided_conv_vs_torch: y, dx, dw, db."""
    from adm_amd import ops_ae
    x = fill.hash_tensor((B, ci, H, W), "dx", 1.0)
    w = fill.hash_tensor((co, ci, 3, 3), "dw", (1.0 / (9 * ci)) ** 0.5)
    b = fill.hash_tensor((co,), "db", 0.1)
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    want = F.conv2d(F.pad(xd, (0, 1, 0, 1)), wd, bd, stride=2)
    dy = fill.hash_tensor(tuple(want.shape), "ddy", 1.0)
    want.backward(dy.double())
    xg = nhwc(x, ci).to(gpu).requires_grad_()
    wg, bg = w.to(gpu).requires_grad_(), b.to(gpu).requires_grad_()
    y = ops_ae.conv2d_down(xg, wg, bg, stride=2, pad_lo=0, pad_hi=1)
    assert y.shape == (B, want.shape[2], want.shape[3], co)
    close(y.permute(0, 3, 1, 2), want)
    y.backward(nhwc(dy, co).to(gpu))
    close(xg.grad.permute(0, 3, 1, 2), xd.grad)
    close(wg.grad, wd.grad)
    close(bg.grad, bd.grad)


def test_posterior_kl_vs_torch(gpu):
    """z, kl and their gradients to the moments, with logvar elements beyond the clamp on both sides (no gradient there)."""
    from adm_amd import ops_ae
    B, H, W, C = 3, 5, 7, 3
    mom = fill.hash_tensor((B, H, W, 32), "pk.mom", 2.0)
    mom[..., C:2 * C] *= 20                                    # logvar in (-40, 40): both clamps are active somewhere
    assert (mom[..., C:2 * C] > 20).any() and (mom[..., C:2 * C] < -30).any()
    eps = fill.hash_tensor((B, H, W, C), "pk.eps", 1.7)
    md = mom.double().requires_grad_()
    mean, lv = md[..., :C], md[..., C:2 * C].clamp(-30.0, 20.0)
    zw = mean + torch.exp(0.5 * lv) * eps.double()
    klw = 0.5 * torch.sum(mean ** 2 + torch.exp(lv) - 1.0 - lv, dim=[1, 2, 3])
    dz, dkl = fill.hash_tensor((B, H, W, C), "pk.dz", 1.0), fill.hash_tensor((B,), "pk.dkl", 1e-3)
    ((zw * dz.double()).sum() + (klw * dkl.double()).sum()).backward()
    mg = mom.to(gpu).requires_grad_()
    z, kl = ops_ae.posterior_sample_kl(mg, C, eps.to(gpu))
    assert z.shape == (B, H, W, 32) and float(z.detach()[..., C:].abs().max()) == 0.0
    close(z[..., :C], zw)
    close(kl, klw)
    dzp = torch.zeros(B, H, W, 32)
    dzp[..., :C] = dz
    torch.autograd.backward([z, kl], [dzp.to(gpu), dkl.to(gpu)])
    close(mg.grad, md.grad)
    assert float(mg.grad[..., 2 * C:].abs().max()) == 0.0
    # kl alone (no dz arrives)
    mg.grad = None
    z, kl = ops_ae.posterior_sample_kl(mg, C, eps.to(gpu))
    kl.sum().backward()
    md.grad = None
    (0.5 * torch.sum(md[..., :C] ** 2 + torch.exp(md[..., C:2 * C].clamp(-30.0, 20.0)) - 1.0 - md[..., C:2 * C].clamp(-30.0, 20.0))).backward()
    close(mg.grad, md.grad)


@pytest.mark.parametrize("shape,with_p", [((2, 3, 16, 16), True), ((3, 3, 5, 7), True), ((2, 3, 64, 48), False)])
def test_nll_vs_torch(gpu, shape, with_p):
    """nll_loss and rec_loss with the reference's broadcast of the [B,1,1,1] LPIPS value over every element, and the gradients to
    the reconstruction, the LPIPS values and logvar.  (3, 3, 5, 7): an element count that is no multiple of four."""
    from adm_amd import ops_ae
    B = shape[0]
    x, r = fill.hash_tensor(shape, "nll.x", 1.0), fill.hash_tensor(shape, "nll.r", 1.0)
    p = fill.hash_tensor((B,), "nll.p", 0.3).abs() if with_p else None
    lv = torch.tensor(0.37)
    rd, lvd = r.double().requires_grad_(), lv.double().requires_grad_()
    pd = p.double().requires_grad_() if with_p else None
    rec = (x.double() - rd).abs() + (x.double() - rd) ** 2
    if with_p:
        rec = rec + 0.8 * pd.reshape(B, 1, 1, 1)
    nll = torch.sum(rec / torch.exp(lvd) + lvd) / B
    (1.7 * nll).backward()
    rg, lvg = r.to(gpu).requires_grad_(), lv.to(gpu).requires_grad_()
    pg = p.to(gpu).requires_grad_() if with_p else None
    out = ops_ae.nll_terms(x.to(gpu), rg, pg, lvg, 0.8)
    close(out[0], nll)
    close(out[1], rec.mean())
    (1.7 * out[0]).backward()
    close(rg.grad, rd.grad)
    close(lvg.grad, lvd.grad)
    if with_p:
        close(pg.grad, pd.grad)


@pytest.mark.parametrize("shape", [(2, 6, 6), (3, 30, 30), (1, 7, 5)])
def test_logit_terms_vs_torch(gpu, shape):
    """mean relu(1 - l), mean relu(1 + l), mean l over channel 0 of the padded logit map; the pad channels hold garbage on purpose:
    they must not contribute and must receive exactly zero gradient."""
    from adm_amd import ops_ae
    B, H, W = shape
    lg = fill.hash_tensor((B, H, W, 32), "lt", 2.5)
    ld = lg[..., 0].double().requires_grad_()
    for fn, ref in ((ops_ae.hinge_real, lambda l: F.relu(1.0 - l).mean()), (ops_ae.hinge_fake, lambda l: F.relu(1.0 + l).mean()),
                    (ops_ae.logit_mean, lambda l: l.mean())):
        ld.grad = None
        want = ref(ld)
        (0.5 * want).backward()
        g = lg.to(gpu).requires_grad_()
        got = fn(g)
        close(got, want)
        (0.5 * got).backward()
        close(g.grad[..., 0], ld.grad, scale=1.0 / (B * H * W), atol=1e-4)
        assert float(g.grad[..., 1:].abs().max()) == 0.0


def test_leaky_relu_vs_torch(gpu):
    from adm_amd import ops_ae
    x = fill.hash_tensor((2, 5, 7, 64), "lr.x", 2.0)
    x[0, 0, 0, :4] = 0.0                                       # the kink: torch gives it the negative slope
    dy = fill.hash_tensor((2, 5, 7, 64), "lr.dy", 1.0)
    xd = x.double().requires_grad_()
    want = F.leaky_relu(xd, 0.2)
    want.backward(dy.double())
    xg = x.to(gpu).requires_grad_()
    y = ops_ae.leaky_relu(xg, 0.2)
    close(y, want)
    y.backward(dy.to(gpu))
    close(xg.grad, xd.grad)


@pytest.mark.parametrize("rows,cols", [(64, 64), (300, 1024), (9, 36), (5, 8192), (3, 8196)])     # > 8192: the two-pass kernel
def test_softmax_rows_bwd_vs_torch(gpu, rows, cols):
    from adm_amd import hip
    s = fill.hash_tensor((rows, cols), "sb.s", 6.0).double().requires_grad_()
    dP = fill.hash_tensor((rows, cols), "sb.dp", 1.0)
    P = torch.softmax(0.37 * s, dim=1)
    P.backward(dP.double())
    Pg, dg = P.detach().float().to(gpu), dP.clone().to(gpu)
    hip.call("adm_softmax_rows_bwd", hip.ptr(Pg), hip.ptr(dg), rows, cols, cols, 0.37)
    close(dg, s.grad, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("rows,cols", [(64, 64), (256, 128), (100, 36), (4, 260)])
def test_transpose2d(gpu, rows, cols):
    from adm_amd import hip
    x = fill.hash_tensor((rows, cols), "tr", 1.0).to(gpu)
    out = torch.full((cols, rows), float("nan"), device=gpu)
    hip.call("adm_transpose2d", hip.ptr(x), hip.ptr(out), rows, cols)
    assert torch.equal(out, x.t().contiguous())


@pytest.mark.parametrize("C,L", [(128, 256), (512, 1024)])
def test_attention_single_head_vs_torch(gpu, C, L):
    """The attention core under autograd: o, dq, dk, dv against fp64 torch."""
    from adm_amd import ops_ae
    B = 2
    q, k, v = (fill.hash_tensor((B, L, C), f"at.{n}", s) for n, s in (("q", 1.5), ("k", 1.5), ("v", 1.0)))
    do = fill.hash_tensor((B, L, C), "at.do", 1.0)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    want = torch.softmax(torch.bmm(qd, kd.transpose(1, 2)) * C ** -0.5, dim=2) @ vd
    want.backward(do.double())
    qg, kg, vg = (t.to(gpu).requires_grad_() for t in (q, k, v))
    o = ops_ae.attention_single_head(qg, kg, vg)
    close(o, want)
    o.backward(do.to(gpu))
    close(qg.grad, qd.grad)
    close(kg.grad, kd.grad)
    close(vg.grad, vd.grad)


@pytest.mark.parametrize("C,hw", [(128, (16, 16)), (512, (32, 32))])
def test_attn_block_vs_oracle_under_autograd(gpu, C, hw):
    """The trainable AttnBlock (GroupNorm, q / k / v / proj_out convs, attention core, residual) against oracle/ae_ref.attn_block
    at fp64 under autograd: output, input gradient and every parameter gradient; C = 128 / L = 256 and C = 512 / L = 1024."""
    from adm_amd.ddm.encoder_decoder import AttnBlock
    shapes = ae_ref._attn_shapes("encoder.mid.attn_1", C)
    sd = fill.filled_state_dict(shapes)
    x = fill.hash_tensor((2, C, *hw), "ab.x", 1.0)
    dy = fill.hash_tensor((2, C, *hw), "ab.dy", 1.0)
    sdd = {k: v.double().requires_grad_() for k, v in sd.items()}
    xd = x.double().requires_grad_()
    want = ae_ref.attn_block(sdd, "encoder.mid.attn_1", xd)
    want.backward(dy.double())
    blk = AttnBlock(C)
    blk.load_state_dict({k[len("encoder.mid.attn_1."):]: v for k, v in sd.items()}, strict=True)
    blk = blk.to(gpu)
    blk.trainable = True
    xg = nhwc(x, C).to(gpu).requires_grad_()
    y = blk(xg)
    close(y.permute(0, 3, 1, 2), want)
    y.backward(nhwc(dy, C).to(gpu))
    close(xg.grad.permute(0, 3, 1, 2), xd.grad)
    for k, p in blk.named_parameters():
        g = sdd["encoder.mid.attn_1." + k].grad
        close(p.grad, g)
        if k == "k.bias":       # exactly zero in exact arithmetic (a constant added to every key shifts a softmax row uniformly)
            assert float(p.grad.abs().max()) <= 1e-4 * float(sdd["encoder.mid.attn_1.q.bias"].grad.abs().max()), k
        else:
            assert rel_l2(p.grad, g) < 2e-3, k


def test_adaptive_weight_and_axpy(gpu):
    """d_weight from two gradient buffers (element counts that are no multiple of four), interior and on both clamps."""
    from adm_amd import ops_ae
    a, b = fill.hash_tensor((3, 37, 3, 3), "aw.a", 0.3), fill.hash_tensor((5, 11), "aw.b", 0.7)
    for sa, sb in ((1.0, 1.0), (1e6, 1e-3), (0.0, 1.0)):
        want = torch.clamp((sa * a.double()).norm() / ((sb * b.double()).norm() + 1e-4), 0.0, 1e4) * 0.5
        got = ops_ae.adaptive_weight((sa * a).to(gpu), (sb * b).to(gpu), 0.5)
        assert got.shape == ()
        close(got, want)
    u, v = fill.hash_tensor((2, 3, 8, 8), "aw.u", 1.0), fill.hash_tensor((2, 3, 8, 8), "aw.v", 1.0)
    coef = torch.tensor(0.731)
    close(ops_ae.axpy_dev(u.to(gpu), v.to(gpu), coef.to(gpu), 0.25), u.double() + 0.731 * 0.25 * v.double())


# ------------------------------------------------------------------------------------------------ discriminator
def _torch_discriminator(sd):
    """The reference's nn.Sequential, rebuilt: 4x4 convs, BatchNorm2d, LeakyReLU(0.2)."""
    seq = []
    layers = R.disc_layers()
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
def test_discriminator_vs_torch(gpu, training):
    """Logits, the gradient at the input, every parameter gradient and the BatchNorm running statistics against fp64 torch;
    48x40 input: odd map sizes after the stride-1 convs (6x5 -> 5x4 -> 4x3)."""
    from adm_amd.ddm.loss import NLayerDiscriminator
    sd = R.disc_state(3.0)
    x = fill.hash_tensor((2, 3, 48, 40), "disc.x", 1.0)
    ref = _torch_discriminator(sd).train(training)
    xd = x.double().requires_grad_()
    want = ref.main(xd)
    dy = fill.hash_tensor(tuple(want.shape), "disc.dy", 1.0)
    want.backward(dy.double())
    D = NLayerDiscriminator().to(gpu).train(training)
    D.load_state_dict(sd, strict=True)
    xg = nhwc(x, 32).to(gpu).requires_grad_()
    y = D(xg)
    assert y.shape == (2, want.shape[2], want.shape[3], 32)
    close(y[..., :1].permute(0, 3, 1, 2), want)
    assert float(y.detach()[..., 1:].abs().max()) == 0.0
    y.backward(nhwc(dy, 32).to(gpu))
    close(xg.grad[..., :3].permute(0, 3, 1, 2), xd.grad)
    rp = dict(ref.named_parameters())
    for k, p in D.named_parameters():
        assert rel_l2(p.grad, rp[k].grad) < 2e-3, k
        close(p.grad, rp[k].grad)
    rs = ref.state_dict()
    for k, v in D.state_dict().items():
        if "running" in k or "num_batches" in k:
            close(v, rs[k], rtol=1e-5, atol=1e-6)
            assert torch.equal(v.cpu().double(), sd[k].double()) == (not training), k        # untouched in eval()


# ------------------------------------------------------------------------------------------------ training steps vs golden
DD = dict(double_z=True, z_channels=3, resolution=list(R.RES), in_channels=3, out_ch=3, ch=R.CH, ch_mult=[1, 2, 4], num_res_blocks=2,
          attn_resolutions=[], dropout=0.0)
STEPS = {"pre": 0, "post": 3, "clamp": 3, "lvclamp": 3}
D_WEIGHT_BAR = 1e-3          # max(1e-3, 4 x 1.1e-5): see test_train_step_vs_golden


def build_trainable(gpu, tag):
    import importlib
    from adm_amd.ddm.lpips import LPIPS
    ED = importlib.import_module("ddm.encoder_decoder")
    ae = ED.AutoencoderKL(DD, dict(R.LOSSCONFIG), 3)
    ae.enable_training(lpips=LPIPS.from_state_dict(lpips_ref.synthetic_state_dict()))
    msg = ae.load_state_dict(R.case_state(tag, torch.float32), strict=False)
    assert not msg.unexpected_keys and all(k.startswith("loss.perceptual_loss.") for k in msg.missing_keys)
    return ae.to(gpu).train()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_ae_train.npz"))


@pytest.mark.parametrize("tag,idx", [("pre", 0), ("pre", 1), ("post", 0), ("post", 1), ("clamp", 0), ("lvclamp", 0)])
def test_train_step_vs_golden(gpu, gold, tag, idx):
    """One training micro-step against the reference's fp64 results (tests/golden/g18_ae_train.npz): log values at rtol 1e-3,
    gradients at 2e-3 relative L2 (a norm on purpose: |x - r|, hinge, LeakyReLU, ReLU and max-pool kinks may flip single elements
    between two correct fp32 implementations), d_weight at max(1e-3, 4 x the fp32-torch deviation) = 1e-3: the host test
    (tests/test_ae_train_host.py) measures that deviation as 4.2e-7 ('pre'), 1.1e-5 ('post') and 4.3e-6 ('lvclamp').
    Measured on an MI355X: d_weight 3.3e-5 / 3.4e-5 / 1e-8 off ('pre' / 'post' / 'lvclamp'), logs <= 1.4e-6, gradients
    <= 9.9e-4 relative L2 ('pre' quant_conv; 'post' 1.0e-4 .. 2.7e-4, next to fp32 torch's own 2.0e-4).
    The step must leave the other optimiser's gradients untouched, and update the BatchNorm statistics once (generator step: one
    discriminator call) or twice (discriminator step: real, then fake)."""
    ae = build_trainable(gpu, tag)
    x, eps = R.case_inputs(tag)
    loss, log = ae.training_step(x.to(gpu), idx, STEPS[tag], eps=eps.to(gpu))
    key = f"{tag}.opt{idx}"
    for k in gold.files:
        if k.startswith(f"{key}.log."):
            name = k[len(key) + 5:]
            got, want = float(log[name]), float(gold[k])
            print(f"{key} {name}: {got:.8g} (golden {want:.8g})")
            bar = D_WEIGHT_BAR if name.endswith("d_weight") else 1e-3
            assert abs(got - want) <= bar * abs(want) + 1e-7, (name, got, want)
            assert isinstance(log[name], torch.Tensor)
    assert abs(float(loss) - float(gold[f"{key}.loss"])) <= 1e-3 * abs(float(gold[f"{key}.loss"])) + 1e-7
    params = dict(ae.named_parameters())
    n = 0
    for k in gold.files:
        if k.startswith(f"{key}.grad."):
            name = k[len(key) + 6:]
            e = rel_l2(params[name].grad, gold[k])
            print(f"{key} grad {name}: rel L2 {e:.2e}")
            assert e < 2e-3, (name, e)
            n += 1
    assert n >= 1
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


def test_eval_mode_and_validation_step_leave_state_alone(gpu):
    """In eval() the BatchNorm statistics do not move; validation_step produces both logs and no gradient anywhere."""
    ae = build_trainable(gpu, "post").eval()
    before = {k: v.clone() for k, v in ae.state_dict().items()}
    x, eps = R.case_inputs("post")
    log_ae, log_disc = ae.validation_step(x.to(gpu), 3, eps=eps.to(gpu))
    assert set(log_ae) == {f"val/{k}" for k in ("total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss")}
    assert set(log_disc) == {"val/disc_loss", "val/logits_real", "val/logits_fake"}
    assert all(torch.isfinite(v).all() for v in list(log_ae.values()) + list(log_disc.values()))
    assert all(p.grad is None for p in ae.parameters())
    after = ae.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


_DET_CHILD = """
import sys, torch
sys.path[:0] = [{root!r}, {tests!r}]
import test_hip_ae_train as T
dev = torch.device('cuda:0')
out = []
for run in range(2):
    res = {{}}
    for idx in (0, 1):
        ae = T.build_trainable(dev, 'post')
        x, eps = T.R.case_inputs('post')
        ae.training_step(x.to(dev), idx, 3, eps=eps.to(dev))
        res.update({{(idx, k): p.grad.clone() for k, p in ae.named_parameters() if p.grad is not None}})
    out.append(res)
assert out[0].keys() == out[1].keys() and len(out[0]) > 200
bad = [k for k in out[0] if not torch.equal(out[0][k], out[1][k])]
print('DETERMINISTIC' if not bad else 'DIFFERS %r' % (bad[:5],))
"""


def test_deterministic_mode_gives_identical_gradients(gpu):
    """ADM_DETERMINISTIC=1 (set for a child process only): two runs of both micro-steps give bit-identical gradients."""
    env = dict(os.environ, ADM_DETERMINISTIC="1", PYTHONPATH=ROOT)
    code = _DET_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "DETERMINISTIC" in r.stdout, r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ driver
def test_cli_train_vae_save_resume_and_use_as_first_stage(gpu, tmp_path):
    """train_vae.py as a child process: 3 steps on synthetic data (ch 32, 64x64, disc_start 2), a checkpoint, a resumed 4th step;
    the checkpoint then loads as the first stage of ddm_const_2.LatentDiffusion through init_from_ckpt ('ema' and 'model')."""
    import importlib
    import math
    import re
    import yaml
    cfg = yaml.load(open(os.path.join(ROOT, "configs", "celebahq", "celeb_ae_kl_256x256_d4.yaml")), Loader=yaml.SafeLoader)
    cfg["model"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["lossconfig"]["disc_start"] = 2
    cfg["data"].update(image_size=[64, 64], batch_size=2)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, train_num_steps=4, save_and_sample_every=3, log_freq=1, ema_update_after_step=1,
                          ema_update_every=1)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train_vae.py"), "--cfg", path]
    r = subprocess.run(cmd + ["--max-steps", "3"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"\[Train Step\] (\d+)/4: (.*) lr=", r.stdout)
    assert [int(l[0]) for l in lines] == [0, 1, 2], r.stdout[-2000:]
    logs = [dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in l[1].split()) for l in lines]
    keys = {"total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss", "disc_loss", "logits_real",
            "logits_fake"}
    assert all(set(lg) == keys and all(math.isfinite(v) for v in lg.values()) for lg in logs), logs
    assert [lg["disc_factor"] for lg in logs] == [0.0, 0.0, 1.0]
    assert logs[0]["disc_loss"] == 0.0 and logs[2]["disc_loss"] > 0.0
    ck_path = os.path.join(res, "model-1.pt")
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert set(ck) == {"step", "model", "opt_ae", "lr_scheduler_ae", "opt_disc", "lr_scheduler_disc", "ema", "scaler"} and ck["step"] == 3
    assert "loss.logvar" in ck["model"] and "ema_model.loss.discriminator.main.0.weight" in ck["ema"]
    assert os.path.exists(os.path.join(res, "sample-1.png"))
    r = subprocess.run(cmd + ["--resume", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = re.findall(r"\[Train Step\] (\d+)/4: (.*) lr=", r.stdout)
    assert [int(l[0]) for l in lines] == [3] and "disc_factor=1 " in lines[0][1], r.stdout[-2000:]
    ED = importlib.import_module("ddm.encoder_decoder")
    D2 = importlib.import_module("ddm.ddm_const_2")
    x = fill.hash_tensor((2, 3, 64, 64), "cli.x", 1.0).to(gpu)
    for use_ema in (True, False):
        fs = ED.AutoencoderKL(cfg["model"]["ddconfig"], cfg["model"]["lossconfig"], 3)
        fs.init_from_ckpt(ck_path, use_ema=use_ema)
        assert fs.loss is None
        key = ("ema_model." if use_ema else "") + "decoder.conv_out.weight"
        assert torch.equal(fs.decoder.conv_out.weight.detach(), (ck["ema"] if use_ema else ck["model"])[key])
    # ... and as the frozen first stage of the latent wrapper (the existing path: AutoencoderKL(ckpt_path=...) -> LatentDiffusion)
    from oracle import unet_ref
    U = importlib.import_module("unet.uncond_unet_sd_2")
    cfg_u = unet_ref.default_cfg(variant="uncond_unet_sd_2", model_channels=64, num_blocks=1, dropout=0.0, img_resolution=16,
                                 attn_resolutions=[8])
    kw = {k: cfg_u[k] for k in ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions", "dropout",
                                "augment_dim")}
    unet = U.EDMPrecond(img_resolution=16, img_channels=3, model_type="DhariwalUNet", **kw)
    first_stage = ED.AutoencoderKL(cfg["model"]["ddconfig"], cfg["model"]["lossconfig"], 3, ckpt_path=ck_path)
    model_cfg = dict(eps=1e-3, sigma_max=1, sigma_min=0.001, weighting_loss=True, use_augment=False, use_disloss=False)
    ldm = D2.LatentDiffusion(auto_encoder=first_stage, scale_factor=1.0, scale_by_std=True, default_scale=False, model=unet,
                             image_size=[64, 64], sampling_timesteps=10, loss_type="l2", start_dist="normal", perceptual_weight=0.0,
                             use_l1=False, cfg=dict(model_cfg)).to(gpu)
    fs = ldm.first_stage_model
    assert all(not p.requires_grad for p in fs.parameters()) and fs.loss is None
    assert torch.equal(fs.decoder.conv_out.weight.detach().cpu(), ck["ema"]["ema_model.decoder.conv_out.weight"])
    post = fs.encode(x)
    z = post.sample()
    assert z.shape == (2, 3, 16, 16) and torch.isfinite(z).all()
    rec = fs.decode(z)
    assert rec.shape == (2, 3, 64, 64) and torch.isfinite(rec).all()
