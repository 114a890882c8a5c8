"""GPU: the single-channel Swin condition encoder and the sketch-to-image recipe on HIP kernels.

The fused stem kernel (adm_patch_embed_ln_fwd: Conv2d(1, E, 4, 4) + LayerNorm in one launch) against the float64 outputs of the
reference's own first_coonv (tests/golden/g25_swin_sci.npz) on ragged, single-column and single-token shapes and on plain,
offset (+300) and all-zero images; its refusals; the backward kernel (adm_patch_embed_ln_bwd: dW, db, dgamma, dbeta, no dX) against
float64 autograd over conv2d -> permute -> layer_norm on the CPU, and its run-to-run bit equality; the one-channel small model and
Swin-B end to end and the train-mode gradients of first_coonv.* against g25; ``Unet(cond_encoder="swin_b", single_channel_cond=True,
train_cond_encoder=True)`` forward and backward against the CPU oracle, and its tensors in ``FlatParams``; ``SketchBatchStream``
against PIL's own resize of the files of a tiny tree; train_cond_ldm.py / sample_cond_ldm.py on scaled-down copies of the two
YAMLs.  Every comparison is at the project's bar (tests/parity.close: rtol 1e-3 / atol 1e-4, scale = max |want| of the tensor).
"""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import swin_ref as R
import swin_sci_ref as C
import swin_train_ref as T
from oracle import cond_unet_ref as CR
from oracle import fill
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def _f32(t, gpu, grad=False):
    return t.detach().to(torch.float32).to(gpu).contiguous().requires_grad_(grad)


# ------------------------------------------------------------------------------------------------ the forward kernel
@pytest.mark.parametrize("content", C.STEM_CONTENTS)
@pytest.mark.parametrize("name", list(C.STEM_CASES))
def test_patch_embed_ln_forward_vs_fp64(gpu, golden, name, content):
    from adm_amd import ops_swin as osw
    B, H, W, E = C.STEM_CASES[name]
    sd = C.stem_params(E)
    x = C.stem_input(name, content)
    y = osw.patch_embed_ln(_f32(x, gpu), *(_f32(sd[k], gpu) for k in C.STEM_NAMES))
    assert tuple(y.shape) == (B, H // 4, W // 4, E) and y.is_contiguous()
    want = C.stem(sd, x)
    print(f"{name}/{content}: max |y - fp64| = {float((y.cpu().double() - want).abs().max()):.3e}")
    close(R.sample(y.cpu()), golden[f"stem.{name}.{content}"])          # the reference's own first_coonv
    close(y, want)                                                        # every element, against the restatement
    if content == "zero":          # conv output = its bias at every token: all rows are the same row
        assert torch.equal(y, y[:1, :1, :1].expand_as(y))


def test_patch_embed_ln_zero_weights_give_the_norm_bias(gpu):
    from adm_amd import ops_swin as osw
    for name in ("s30x44", "s64x64"):
        B, H, W, E = C.STEM_CASES[name]
        sd = C.stem_params(E, torch.float32)
        x = C.stem_input(name, "offset", torch.float32).to(gpu)
        y = osw.patch_embed_ln(x, torch.zeros(E, 1, 4, 4, device=gpu), torch.zeros(E, device=gpu),
                               sd["first_coonv.2.weight"].to(gpu), sd["first_coonv.2.bias"].to(gpu))
        assert torch.equal(y, sd["first_coonv.2.bias"].to(gpu).expand_as(y))


def test_patch_embed_ln_never_reads_trailing_rows_and_columns(gpu):
    """30 x 44 -> 7 x 11 tokens of rows 0..27: NaNs in rows 28, 29 change nothing; an unaligned width takes the by-element loads."""
    from adm_amd import ops_swin as osw
    sd = [_f32(v, gpu) for v in C.stem_params(32).values()]
    x = C.stem_input("s30x44", "plain", torch.float32)
    a = osw.patch_embed_ln(x.to(gpu), *sd)
    x2 = x.clone()
    x2[:, :, 28:] = float("nan")
    assert torch.equal(osw.patch_embed_ln(x2.to(gpu), *sd), a)
    x3 = torch.full((2, 1, 30, 47), float("nan"))          # W % 4 == 3
    x3[..., :44] = x
    x3[:, :, 28:] = float("nan")
    assert torch.equal(osw.patch_embed_ln(x3.to(gpu), *sd), a)


def test_patch_embed_ln_refusals(gpu):
    from adm_amd import ops_swin as osw

    def run(E, shape, grad=False):
        sd = [_f32(v, gpu) for v in C.stem_params(E).values()]
        return osw.patch_embed_ln(torch.zeros(*shape, device=gpu).requires_grad_(grad), *sd)

    with pytest.raises(RuntimeError, match="-22|failed"):
        run(48, (1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="-22|failed"):
        run(32, (1, 1, 3, 8))
    with pytest.raises(RuntimeError, match="-22|failed"):
        run(32, (1, 1, 8, 3))
    with pytest.raises(RuntimeError, match="-22|failed"):
        run(544, (1, 1, 8, 8))          # past the bound that is built (512)
    with pytest.raises(RuntimeError, match="1 channel"):
        run(32, (1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no gradient for its input"):
        run(32, (1, 1, 8, 8), grad=True)


# ------------------------------------------------------------------------------------------------ the backward kernel
def _stem_backward(name, gpu):
    from adm_amd import ops_swin as osw
    B, H, W, E = C.STEM_BWD_CASES[name]
    sd = C.stem_params(E)
    x = C.stem_input(name, "plain", cases=C.STEM_BWD_CASES)
    dy = T.weight_like(torch.empty(B, H // 4, W // 4, E), f"sci.stem.{name}.dy")
    ps = [_f32(sd[k], gpu, True) for k in C.STEM_NAMES]
    osw.patch_embed_ln(_f32(x, gpu), *ps).backward(_f32(dy, gpu))
    return [p.grad for p in ps], (sd, x, dy)


@pytest.mark.parametrize("name", list(C.STEM_BWD_CASES))
def test_patch_embed_ln_backward_vs_fp64_autograd(gpu, name):
    got, (sd, x, dy) = _stem_backward(name, gpu)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    want = torch.autograd.grad((C.stem(leaves, x) * dy).sum(), [leaves[k] for k in C.STEM_NAMES])
    for k, g, w in zip(C.STEM_NAMES, got, want):
        assert g is not None and g.shape == w.shape, k
        print(f"{name}/{k}: max err {float((g.cpu().double() - w).abs().max()):.3e} of scale {float(w.abs().max()):.3e}")
        close(g, w)
    again, _ = _stem_backward(name, gpu)
    assert all(torch.equal(a, b) for a, b in zip(got, again))          # fixed-order sums: the same bits every run


# ------------------------------------------------------------------------------------------------ the models
def _model(cfg, gpu):
    from adm_amd.unet.swin_transformer import SwinTransformer
    m = SwinTransformer(patch_size=[4, 4], embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]),
                        window_size=[7, 7], in_chans=1)
    m.load_state_dict(C.filled_state_dict(**cfg, dtype=torch.float32), strict=True)
    return m.to(gpu)


@pytest.mark.parametrize("tag,cfg,name,shape", [("small", R.SMALL, "small", C.SMALL_INPUT), ("swin_b", R.SWIN_B, "b64", C.SWIN_B_INPUT)])
def test_one_channel_model_end_to_end(gpu, golden, tag, cfg, name, shape):
    m = _model(cfg, gpu).eval()
    feats = m(C.model_input(name, shape, torch.float32).to(gpu))
    assert [list(f.shape) for f in feats] == golden[f"{name}.shapes"].tolist()
    for i, f in enumerate(feats):
        assert not f.requires_grad
        close(R.sample(f.cpu()), golden[f"{name}.stage{i}"])
    with pytest.raises(RuntimeError, match="1 channels"):
        m(torch.zeros(1, 3, 32, 32, device=gpu))


@pytest.mark.parametrize("tag,p,keep", C.TRAIN_TAGS, ids=[t[0] for t in C.TRAIN_TAGS])
def test_stem_gradients_through_the_small_model(gpu, golden, tag, p, keep):
    m = _model(R.SMALL, gpu).enable_training(p).train()
    x = C.model_input("small", C.SMALL_INPUT, torch.float32).to(gpu)
    feats = m(x) if keep is None else m(x, keep=keep.to(torch.float32).to(gpu))
    sum((f * T.weight_like(f, f"{tag}.stage{i}").to(f)).sum() for i, f in enumerate(feats)).backward()
    params = dict(m.named_parameters())
    for k in C.STEM_NAMES:
        assert params[k].grad is not None and params[k].grad.shape == params[k].shape, k
        close(T.sample_grad(params[k].grad.cpu()), golden[f"{tag}.{k}"])


# ------------------------------------------------------------------------------------------------ the denoiser
def _cond_unet(gpu, **kw):
    U = importlib.import_module("unet.cond_unet")
    cfg = CR.default_cfg(dim=32, two_decoders=True)
    unet = U.Unet(dim=32, dim_mults=cfg["dim_mults"], cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=1,
                  window_sizes1=cfg["window_sizes1"], window_sizes2=cfg["window_sizes2"], fourier_scale=16, cfg={"cond_net": "swin"},
                  cond_encoder="swin_b", single_channel_cond=True, **kw)
    sd = CR.filled_state_dict(cfg)
    msg = unet.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys and all(k.startswith("init_conv_mask.") for k in msg.missing_keys)
    unet.init_conv_mask.load_state_dict(C.filled_state_dict(**R.SWIN_B, dtype=torch.float32), strict=True)
    return unet.to(gpu).eval(), cfg, sd          # (eval: no dropout and no stochastic-depth draws, so the CPU oracle can follow)


def test_unet_with_the_one_channel_encoder_vs_cpu_oracle(gpu):
    """32x32 latents and a 32x32 one-channel sketch, B = 2, two decoders, the encoder trained along: x1, x2 and the gradients of
    first_coonv.* against the CPU oracle (tests/swin_sci_ref.py in float64 into oracle.cond_unet_ref); then the flat buffer."""
    from adm_amd.optim import FlatParams
    from adm_amd.unet.swin_transformer import SwinTransformer
    unet, cfg, usd = _cond_unet(gpu, train_cond_encoder=True)
    enc = unet.init_conv_mask
    assert isinstance(enc, SwinTransformer) and enc.trainable and enc.in_chans == 1
    assert tuple(enc.first_coonv[0].weight.shape) == (128, 1, 4, 4)
    B = 2
    cond = fill.hash_tensor((B, 1, 32, 32), "sci.cond", 1.0)
    x = fill.hash_tensor((B, 3, 32, 32), "sci.train.x", 1.0)
    t = torch.tensor([0.3, 0.7])
    w1, w2 = (fill.hash_tensor((B, 3, 32, 32), f"sci.train.{k}", 1.0) for k in ("w1", "w2"))
    # the oracle: the encoder restated in float64, the denoiser's oracle in its own float32
    esd = C.filled_state_dict(**R.SWIN_B)
    for k in C.STEM_NAMES:
        esd[k] = esd[k].clone().requires_grad_(True)
    hm = [f.to(torch.float32) for f in C.forward(esd, cond.double(), R.SWIN_B["depths"], R.SWIN_B["num_heads"])]
    o1, o2 = CR.unet_forward(usd, cfg, x, t, hm)
    want = torch.autograd.grad((o1 * w1).sum() + (o2 * w2).sum(), [esd[k] for k in C.STEM_NAMES])
    x1, x2 = unet(x.to(gpu), t.to(gpu), cond.to(gpu))
    close(x1, o1)
    close(x2, o2)
    ((x1 * w1.to(gpu)).sum() + (x2 * w2.to(gpu)).sum()).backward()
    params = dict(enc.named_parameters())
    ga = {k: params[k].grad.clone() for k in C.STEM_NAMES}
    for k, w in zip(C.STEM_NAMES, want):
        print(f"{k}: max err {float((ga[k].cpu().double() - w).abs().max()):.3e} of scale {float(w.abs().max()):.3e}")
        close(ga[k], w)
    assert all(params[k].grad is None for k in ("norm.weight", "head.weight"))
    # the flat buffer holds the one-channel stem; the backward kernel accumulates straight into it
    for p in unet.parameters():
        p.grad = None
    flat = FlatParams(unet)
    names = [n for n, _ in unet.named_parameters()]
    assert "init_conv_mask.first_coonv.0.weight" in names
    w = dict(unet.named_parameters())["init_conv_mask.first_coonv.0.weight"]
    assert tuple(w.shape) == (128, 1, 4, 4) and any(w is q for q in flat.params) and getattr(w, "_adm_direct", False)
    lo, hi = flat.flat.data_ptr(), flat.flat.data_ptr() + 4 * flat.numel
    assert all(lo <= params[k].data_ptr() < hi for k in C.STEM_NAMES)
    flat.zero_grad()
    x1, x2 = unet(x.to(gpu), t.to(gpu), cond.to(gpu))
    ((x1 * w1.to(gpu)).sum() + (x2 * w2.to(gpu)).sum()).backward()
    torch.cuda.synchronize()
    glo, ghi = flat.grad.data_ptr(), flat.grad.data_ptr() + 4 * flat.numel
    for k in C.STEM_NAMES:
        assert glo <= params[k].grad.data_ptr() < ghi          # still the flat gradient buffer: nothing was re-assigned by autograd
        close(params[k].grad, ga[k])


# ------------------------------------------------------------------------------------------------ the batch source
SIZES = [((40, 52), (40, 52)), ((96, 64), (48, 32)), ((64, 64), (64, 64)), ((70, 90), (90, 70))]          # (photo, sketch) per pair


def sketch_tree(root, splits=("train", "val")):
    """GT/{split}/c{k}/img_i.png + Sketch/{split}/c{k}/img_i.png, of different sizes per pair (a sketch need not have its photo's).
    Returns {split: [(photo uint8 [h,w,3], sketch uint8 [h,w])]} in sorted path order, as PIL reads the files back."""
    from PIL import Image
    import duts_data_ref as D
    back = {}
    for split in splits:
        back[split] = []
        for i, (psz, ssz) in enumerate(SIZES):
            sub = f"c{i % 2}"
            for kind in ("GT", "Sketch"):
                os.makedirs(os.path.join(root, kind, split, sub), exist_ok=True)
            Image.fromarray(D.hash_bytes((*psz, 3), f"sk.tree.{split}.p{i}")).save(os.path.join(root, "GT", split, sub, f"img_{i}.png"))
            Image.fromarray(D.hash_bytes(ssz, f"sk.tree.{split}.s{i}")).save(os.path.join(root, "Sketch", split, sub, f"img_{i}.png"))
        open(os.path.join(root, "GT", split, "c0", "._img_0.png"), "wb").write(b"resource fork")          # skipped by name
        order = sorted(range(len(SIZES)), key=lambda i: (f"c{i % 2}", f"img_{i}.png"))
        for i in order:
            sub = f"c{i % 2}"
            back[split].append((np.asarray(Image.open(os.path.join(root, "GT", split, sub, f"img_{i}.png")).convert("RGB")),
                                np.asarray(Image.open(os.path.join(root, "Sketch", split, sub, f"img_{i}.png")).convert("L"))))
    return back


def test_sketch_batch_stream_bytes_are_pils(gpu, tmp_path):
    from PIL import Image
    from adm_amd.ddm.pair_data import SketchBatchStream
    import duts_data_ref as D
    back = sketch_tree(str(tmp_path / "sk"))["train"]
    size = (48, 56)
    stream = SketchBatchStream({"class_name": "ddm.data.SketchDataset", "data_root": str(tmp_path / "sk"), "split": "train",
                                "augment_horizontal_flip": True}, 4, size, gpu, seed=3)
    assert stream.pool.n == 4 and stream.names == ["img_0.png", "img_2.png", "img_1.png", "img_3.png"]
    idx, flip = [3, 0, 1, 2], [1, 0, 0, 1]
    batch = stream.next_batch(idx=idx, flip=flip, want_u8=True)
    assert tuple(batch["image"].shape) == (4, 3, 48, 56) and tuple(batch["cond"].shape) == (4, 1, 48, 56)
    assert set(batch) == {"image", "cond", "image_u8", "cond_u8"}
    for b, (i, f) in enumerate(zip(idx, flip)):
        photo, sketch = back[i]
        rgb = np.asarray(Image.fromarray(photo).resize((size[1], size[0]), Image.BILINEAR))          # PIL's own (antialiased) resize
        gray = np.asarray(Image.fromarray(sketch).resize((size[1], size[0]), Image.BILINEAR))
        if f:
            rgb, gray = rgb[:, ::-1], gray[:, ::-1]
        assert np.array_equal(batch["image_u8"][b].cpu().numpy(), rgb), (b, i)
        assert np.array_equal(batch["cond_u8"][b].cpu().numpy(), gray), (b, i)
        assert torch.equal(batch["image"][b].cpu(), D.to_float(np.ascontiguousarray(rgb)))
        assert torch.equal(batch["cond"][b].cpu(), D.gray_to_float(np.ascontiguousarray(gray)[None])[0])
    # split: test reads val, in order, unflipped, with names
    test = SketchBatchStream({"class_name": "ddm.data.SketchDataset", "data_root": str(tmp_path / "sk"), "split": "test"}, 2, size, gpu, 3)
    tb = test.next_batch()
    assert tb["img_name"] == ["img_0.png", "img_2.png"] and tb["ori_size"] == [(40, 52), (64, 64)]
    assert tuple(tb["cond"].shape) == (2, 1, 48, 56)
    # the synthetic pool of the shipped YAML, through train_cond_ldm.batch_stream
    from train_cond_ldm import batch_stream
    syn = batch_stream({"class_name": "synthetic", "synthetic_of": "ddm.data.SketchDataset", "split": "train"}, 2, size, gpu, 3)
    assert isinstance(syn, SketchBatchStream)
    sb = next(syn)
    assert tuple(sb["image"].shape) == (2, 3, 48, 56) and tuple(sb["cond"].shape) == (2, 1, 48, 56)


# ------------------------------------------------------------------------------------------------ the drivers
def reduced_cfgs(tmp_path):
    out = []
    res = str(tmp_path / "run")
    for name in ("sketchcoco_cond_ddm_const_ldm.yaml", "sketchcoco_cond_ddm_const_ldm_sample.yaml"):
        cfg = yaml.load(open(os.path.join(ROOT, "configs/sketch2img", name)), Loader=yaml.SafeLoader)
        u = cfg["model"]["unet"]
        assert u["single_channel_cond"] is True and u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True
        assert u["class_name"] == "unet.cond_unet.Unet" and u["dim"] == 128 and "use_disloss" not in cfg["model"]
        cfg["model"].update(image_size=[128, 128], sampling_timesteps=2)
        cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[128, 128])
        u.update(dim=32, cond_feature_size=[32, 32])
        cfg["data"].update(class_name="synthetic", synthetic_of="ddm.data.SketchDataset", image_size=[128, 128], batch_size=2)
        cfg["trainer"].update(results_folder=res, gradient_accumulate_every=2, train_num_steps=3, save_and_sample_every=2, log_freq=1,
                              test_before=True, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
        out.append(cfg)
    out[1]["sampler"].update(sample_num=2, ckpt_path=os.path.join(res, "model-1.pt"), save_folder=os.path.join(res, "png"),
                             crop_size=[128, 128], stride=[128, 128])
    return out[0], out[1], res


def test_train_and_sample_sketch_cli_end_to_end(gpu, tmp_path):
    from PIL import Image
    train, sample, res = reduced_cfgs(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    path = str(tmp_path / "train.yaml")
    yaml.safe_dump(train, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_cond_ldm.py"), "--cfg", path,
                        "--max-steps", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/3: loss=(\S+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    assert "sketch pool: 32 pairs" in r.stdout
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert ck["step"] == 2 and tuple(ck["model"]["model.init_conv_mask.first_coonv.0.weight"].shape) == (128, 1, 4, 4)
    for name in ("sample-0_2.png", "sample-1.png"):          # B = 2: one column, two rows; the generated photos are RGB
        im = Image.open(os.path.join(res, name))
        assert im.mode == "RGB" and im.size == (128, 256), (name, im.mode, im.size)
    path = str(tmp_path / "sample.yaml")
    yaml.safe_dump(sample, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "PSNR" not in r.stdout and "2 images in" in r.stdout, r.stdout[-1000:]
    names = sorted(os.listdir(os.path.join(res, "png")))
    assert names == [f"{i:010d}.png" for i in range(2)], names
    for n in names:
        im = Image.open(os.path.join(res, "png", n))
        assert im.mode == "RGB" and im.size == (128, 128), (n, im.mode, im.size)
