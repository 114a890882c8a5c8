"""GPU: the backward pass and stochastic depth of the Swin condition encoder on HIP kernels, against float64 autograd on the CPU
over tests/swin_ref.py / tests/swin_train_ref.py (whose gradients tests/test_swin_train_host.py pins to the reference's own
classes through tests/golden/g20_swin_train.npz): the window-attention gradient on every attention case (padding keys send
their dK / dV to the qkv bias), its run-to-run bit equality, the two LayerNorm gradients, ``row_scale_add``, the small model
with and without injected drops, Swin-B after one backward, and the wiring of ``Unet(..., train_cond_encoder=True)`` into
``FlatParams`` / ``FusedAdamWEMA``.  Every comparison is at the project's bar (tests/parity.close: rtol 1e-3 / atol 1e-4, scale
= max |want| of the tensor)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import swin_ref as R
import swin_train_ref as T
from oracle import fill
from oracle import cond_unet_ref as CR
from parity import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _f32(t, gpu, grad=False):
    return t.detach().to(torch.float32).to(gpu).contiguous().requires_grad_(grad)


# ------------------------------------------------------------------------------------------------ 1, 2: attention
def _attn_backward(name, gpu):
    from adm_amd import ops_swin as osw
    qkv, qb, table, heads, shift = R.attn_case_core(name)
    d_out = T.weight_like(torch.empty(*qkv.shape[:3], qkv.shape[3] // 3), f"attn.{name}.d_out")
    q, b, t = _f32(qkv, gpu, True), _f32(qb, gpu, True), _f32(table, gpu, True)
    out = osw.window_attention(q, b, t, heads, shift)
    out.backward(_f32(d_out, gpu))
    return q.grad, b.grad, t.grad


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_window_attention_backward_vs_fp64(gpu, name):
    want_qkv, want_qb, want_table, _ = T.attn_core_grads(name)
    d_qkv, d_qb, d_table = _attn_backward(name, gpu)
    close(d_qkv, want_qkv)
    close(d_table, want_table)
    close(d_qb, want_qb)
    C = d_qb.numel() // 3
    if name in ("a5x5", "a9x10"):          # padding tokens are keys and values (their k, v ARE the bias), never queries
        assert float(d_qb[C:2 * C].abs().max()) > 0 and float(d_qb[2 * C:].abs().max()) > 0
        assert float(d_qb[:C].abs().max()) == 0.0
    if name == "a14x14":                   # no padding: nothing reaches the bias through the core
        assert float(d_qb.abs().max()) == 0.0


def test_window_attention_backward_is_bit_reproducible(gpu):
    for name in ("a9x10", "a8x8"):
        a, b = _attn_backward(name, gpu), _attn_backward(name, gpu)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_training_path_refuses_the_bf16_mode(gpu):
    from adm_amd import ops, ops_swin as osw
    x = torch.zeros(4, 32, device=gpu, requires_grad=True)
    w, b = torch.ones(32, device=gpu), torch.zeros(32, device=gpu)
    ops.set_compute_precision("bf16")
    try:
        with pytest.raises(NotImplementedError, match="f32 compute mode"):
            osw.layer_norm(x, w, b)
        osw.layer_norm(x.detach(), w, b)          # the no-grad path is untouched
    finally:
        ops.set_compute_precision("f32")


# ------------------------------------------------------------------------------------------------ 3, 4: LayerNorm
@pytest.mark.parametrize("C", [32, 128, 512, 1024, 2048])
def test_layer_norm_backward(gpu, C):
    """The rows of test_layer_norm_affine: plain, on a common offset, sparse, constant (37 rows: each wave walks several)."""
    from adm_amd import ops_swin as osw
    M = 37
    x = fill.hash_tensor((M, C), f"ln.x{C}", 1.0, torch.float64)
    x[5:12] += 300.0
    x[12:15] -= 1000.0
    x[15:20] = 0.0
    x[15:20, 3] = 2.5
    x[17, C - 1] = -40.0
    x[20] = 7.0
    x = x.to(torch.float32)
    w = 1.0 + fill.hash_tensor((C,), f"ln.w{C}", 0.1, torch.float64)
    b = fill.hash_tensor((C,), f"ln.b{C}", 0.1, torch.float64)
    dy = fill.hash_tensor((M, C), f"ln.dy{C}", 1.0, torch.float64)
    xr, wr, br = x.double().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = torch.autograd.grad((R.layer_norm(xr, wr, br) * dy).sum(), [xr, wr, br])
    xg, wg, bg = _f32(x, gpu, True), _f32(w, gpu, True), _f32(b, gpu, True)
    osw.layer_norm(xg, wg, bg).backward(_f32(dy, gpu))
    assert bool(torch.isfinite(xg.grad[20]).all())          # the constant row: rstd = eps ** -0.5
    close(xg.grad, want[0])
    close(wg.grad, want[1])
    close(bg.grad, want[2])


@pytest.mark.parametrize("name", list(R.MERGE_CASES))
def test_merge_layer_norm_backward(gpu, name):
    from adm_amd import ops_swin as osw
    x, sd = R.merge_case_inputs(name)
    w, b = sd[name + ".norm.weight"], sd[name + ".norm.bias"]
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = R.merge_ln(xr, wr, br)
    dy = T.weight_like(y, f"merge.{name}.ln.dy")
    want = torch.autograd.grad((y * dy).sum(), [xr, wr, br])
    xg, wg, bg = _f32(x, gpu, True), _f32(w, gpu, True), _f32(b, gpu, True)
    osw.merge_layer_norm(xg, wg, bg).backward(_f32(dy, gpu))
    assert tuple(xg.grad.shape) == R.MERGE_CASES[name]
    close(xg.grad, want[0])
    close(wg.grad, want[1])
    close(bg.grad, want[2])


# ------------------------------------------------------------------------------------------------ 5: stochastic depth
def test_row_scale_add(gpu):
    from adm_amd import ops_swin as osw
    shape = (3, 5, 6, 32)
    x = fill.hash_tensor(shape, "rsa.x", 1.0, torch.float64).to(torch.float32)
    x[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 1e-30, -3.5])          # a dropped row keeps even the sign of a zero
    r = fill.hash_tensor(shape, "rsa.r", 2.0, torch.float64).to(torch.float32)
    dy = fill.hash_tensor(shape, "rsa.dy", 1.0, torch.float64).to(torch.float32)
    s = torch.tensor([0.0, 2.0, 1.0])
    xg, rg = _f32(x, gpu, True), _f32(r, gpu, True)
    y = osw.row_scale_add(xg, rg, s.to(gpu))
    y.backward(dy.to(gpu))
    sv = s.double().view(3, 1, 1, 1)
    close(y, x.double() + sv * r.double())
    assert torch.equal(y[0].detach().cpu().view(torch.int32), x[0].view(torch.int32))
    close(xg.grad, dy.double())
    assert torch.equal(xg.grad.cpu(), dy)
    close(rg.grad, sv * dy.double())
    assert float(rg.grad[0].abs().max()) == 0.0
    with torch.no_grad():                                              # the no-grad path: the same kernel
        assert torch.equal(osw.row_scale_add(xg, rg, s.to(gpu)), y)


@pytest.mark.parametrize("coff", [3, 8])
def test_bilinear_into_carries_the_condition_gradient(gpu, coff):
    """The stem writes the up-sampled first stage map next to the latent (from channel 3 on): with a trainable encoder that
    write has a gradient."""
    from adm_amd import ops_cond as oc
    x = fill.hash_tensor((2, 3, 4, 32), "bil.x", 1.0, torch.float64)
    dy = fill.hash_tensor((2, 12, 16, 64), "bil.dy", 1.0, torch.float64)
    xr = x.clone().requires_grad_(True)
    up = F.interpolate(xr.permute(0, 3, 1, 2), size=(12, 16), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    want = torch.autograd.grad((up * dy[..., coff:coff + 32]).sum(), xr)[0]
    xg = _f32(x, gpu, True)
    base = torch.zeros(2, 12, 16, 64, device=gpu)
    y = oc.bilinear_into(xg, base, coff, False)
    close(y[..., coff:coff + 32], up)
    y.backward(_f32(dy, gpu))
    close(xg.grad, want)
    plain = oc.bilinear_into(xg.detach(), torch.zeros(2, 12, 16, 64, device=gpu), coff, False)          # the no-grad path as before
    assert torch.equal(plain, y.detach())


# ------------------------------------------------------------------------------------------------ 6: the small model
def _model(cfg, gpu):
    from adm_amd.unet.swin_transformer import SwinTransformer
    m = SwinTransformer(patch_size=[4, 4], embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]),
                        window_size=[7, 7])
    m.load_state_dict(R.filled_state_dict(**cfg, dtype=torch.float32), strict=True)
    return m.to(gpu)


def _backward(m, x, tag, keep=None):
    for p in m.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    feats = m(x) if keep is None else m(x, keep=keep)
    loss = sum((f * T.weight_like(f, f"{tag}.stage{i}").to(f)).sum() for i, f in enumerate(feats))
    loss.backward()
    return feats, x.grad


def _check_grads(m, want, xgrad):
    names = [k for k in want if k != "x"]
    params = dict(m.named_parameters())
    assert sorted(names) == sorted(k for k, p in params.items() if p.requires_grad)
    for k in names:
        assert params[k].grad is not None, k
        close(params[k].grad, want[k])
    close(xgrad, want["x"])
    assert all(params[k].grad is None for k in ("norm.weight", "norm.bias", "head.weight", "head.bias"))


@pytest.fixture(scope="module")
def small_frozen_outputs(gpu):
    m = _model(R.SMALL, gpu).eval()
    return [f.clone() for f in m(R.model_input("small", R.SMALL_INPUT, torch.float32).to(gpu))]


def test_small_model_gradients(gpu, small_frozen_outputs):
    m = _model(R.SMALL, gpu).enable_training(0.0).train()
    x = R.model_input("small", R.SMALL_INPUT, torch.float32).to(gpu)
    feats, xg = _backward(m, x, "small.sd0")
    assert all(torch.equal(a, b) for a, b in zip(feats, small_frozen_outputs))          # p = 0: the frozen module's kernels
    _check_grads(m, T.model_grads(R.SMALL, R.SMALL_INPUT, "small", "small.sd0"), xg)


def test_small_model_gradients_with_stochastic_depth(gpu, small_frozen_outputs):
    m = _model(R.SMALL, gpu).enable_training(0.5).train()
    x = R.model_input("small", R.SMALL_INPUT, torch.float32).to(gpu)
    keep = T.KEEP_SMALL.to(torch.float32).to(gpu)
    feats, xg = _backward(m, x, "small.sd5", keep)
    sd = R.filled_state_dict(**R.SMALL)
    scales = T.scales_from_keep(T.KEEP_SMALL, T.sd_probs(R.SMALL["depths"], 0.5))
    for f, w in zip(feats, T.forward(sd, R.model_input("small", R.SMALL_INPUT), R.SMALL["depths"], R.SMALL["num_heads"], scales)):
        close(f, w)
    assert not torch.equal(feats[-1], small_frozen_outputs[-1])
    _check_grads(m, T.model_grads(R.SMALL, R.SMALL_INPUT, "small", "small.sd5", T.KEEP_SMALL, 0.5), xg)
    # draws from the device generator: reproducible under a seed, and a wrong shape is refused
    torch.manual_seed(5)
    a = m(x)
    torch.manual_seed(5)
    b = m(x)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    with pytest.raises(RuntimeError, match="keep must be"):
        m(x, keep=keep[:, :, :1])
    # eval: the identity path, bit for bit the frozen module's outputs (with grad enabled)
    m.eval()
    assert all(torch.equal(p, q) for p, q in zip(m(x), small_frozen_outputs))
    assert all(torch.equal(p, q) for p, q in zip(m(x, keep=keep), small_frozen_outputs))


# ------------------------------------------------------------------------------------------------ 7: Swin-B
def test_swin_b_gradients_after_one_backward(gpu):
    names = ["first_coonv.0.weight", "features.4.17.attn.relative_position_bias_table", "features.6.1.mlp.3.weight"]
    shape = R.SWIN_B_INPUTS["b64"]
    sd = R.filled_state_dict(**R.SWIN_B)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    feats = T.forward(sd, R.model_input("b64", shape), R.SWIN_B["depths"], R.SWIN_B["num_heads"])
    want = torch.autograd.grad(T.model_loss(feats, "b64"), [sd[k] for k in names])
    del feats
    m = _model(R.SWIN_B, gpu).enable_training(0.0).train()
    _backward(m, R.model_input("b64", shape, torch.float32).to(gpu), "b64")
    params = dict(m.named_parameters())
    for k, w in zip(names, want):
        close(params[k].grad, w)
    for k, p in params.items():
        if k.startswith(("norm.", "head.")):
            assert p.grad is None
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


# ------------------------------------------------------------------------------------------------ 8: wiring
def _cond_unet(gpu, **kw):
    U = importlib.import_module("unet.cond_unet")
    cfg = CR.default_cfg(dim=32, two_decoders=True)
    unet = U.Unet(dim=32, dim_mults=cfg["dim_mults"], cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=3,
                  window_sizes1=cfg["window_sizes1"], window_sizes2=cfg["window_sizes2"], fourier_scale=16, cfg={"cond_net": "swin"},
                  cond_encoder="swin_b", **kw)
    msg = unet.load_state_dict(CR.filled_state_dict(cfg), strict=False)
    assert not msg.unexpected_keys and all(k.startswith("init_conv_mask.") for k in msg.missing_keys)
    unet.init_conv_mask.load_state_dict(R.filled_state_dict(**R.SWIN_B, dtype=torch.float32), strict=True)
    return unet.to(gpu).eval()          # (eval: the denoiser's own dropout would differ from run to run)


def test_train_cond_encoder_wiring(gpu):
    """32x32 latents and a 32x32 condition image, B = 2, two decoders: the geometry of
    test_two_step_sample_through_the_builtin_encoder."""
    from adm_amd.optim import FlatParams, FusedAdamWEMA
    from adm_amd.unet.swin_transformer import SwinTransformer
    unet = _cond_unet(gpu, train_cond_encoder=True)
    enc = unet.init_conv_mask
    assert isinstance(enc, SwinTransformer) and enc.trainable and enc.blocks()[-1].sd_prob == 0.5
    enc.train()                          # stochastic depth on; its draws come from the seeded device generator
    B = 2
    cond = fill.hash_tensor((B, 3, 32, 32), "swin.cond", 1.0).to(gpu)
    x = fill.hash_tensor((B, 3, 32, 32), "swin.train.x", 1.0).to(gpu)
    t = torch.tensor([0.3, 0.7], device=gpu)
    w1 = fill.hash_tensor((B, 3, 32, 32), "swin.train.w1", 1.0).to(gpu)
    w2 = fill.hash_tensor((B, 3, 32, 32), "swin.train.w2", 1.0).to(gpu)
    names = [k for k, p in enc.named_parameters() if p.requires_grad]
    params = dict(enc.named_parameters())

    def loss_of(mask):
        x1, x2 = unet(x, t, mask)
        return (x1 * w1).sum() + (x2 * w2).sum()

    def clear():
        for p in unet.parameters():
            p.grad = None

    # A: one loss backward through denoiser and encoder
    torch.manual_seed(11)
    loss_of(cond).backward()
    ga = {k: params[k].grad.clone() for k in names}
    assert all(bool(torch.isfinite(g).all()) for g in ga.values())
    assert float(ga["first_coonv.0.weight"].abs().max()) > 0
    assert all(params[k].grad is None for k in ("norm.weight", "head.weight"))
    # B: the same draws, the stage maps given as leaves -> dL/d(stage map)
    clear()
    torch.manual_seed(11)
    with torch.no_grad():
        feats = enc(cond)
    leaves = [f.detach().clone().requires_grad_(True) for f in feats]
    loss_of(leaves).backward()
    assert all(params[k].grad is None for k in names)
    # C: the encoder alone, driven by those
    clear()
    torch.manual_seed(11)
    torch.autograd.backward(enc(cond), [l.grad for l in leaves])
    for k in names:
        close(ga[k], params[k].grad)
    # the flat buffer holds the encoder's tensors, the kernels accumulate straight into it, the fused step moves them
    clear()
    flat = FlatParams(unet)
    lo, hi = flat.flat.data_ptr(), flat.flat.data_ptr() + 4 * flat.numel
    assert all(lo <= params[k].data_ptr() < hi and getattr(params[k], "_adm_direct", False) for k in names)
    assert not any(p is q for q in flat.params for p in (enc.norm.weight, enc.head.weight))
    flat.zero_grad()
    torch.manual_seed(11)
    loss_of(cond).backward()
    torch.cuda.synchronize()
    for k in ("first_coonv.0.weight", "first_coonv.2.weight", "features.0.1.attn.qkv.bias", "features.4.17.attn.relative_position_bias_table",
              "features.5.norm.bias", "features.6.1.mlp.3.weight"):
        close(params[k].grad, ga[k])
    before = flat.flat.clone()
    FusedAdamWEMA(flat, lr=1e-3).step()
    torch.cuda.synchronize()
    off = dict(zip((id(p) for p in flat.params), flat.offsets))
    for k in names:
        o, n = off[id(params[k])], params[k].numel()
        assert not torch.equal(flat.flat[o:o + n], before[o:o + n]), k
    o, n = off[id(params["first_coonv.0.weight"])], params["first_coonv.0.weight"].numel()
    assert torch.equal(params["first_coonv.0.weight"].detach().reshape(-1), flat.flat[o:o + n])


def test_without_the_flag_the_encoder_stays_frozen(gpu):
    from adm_amd.optim import FlatParams
    unet = _cond_unet(gpu)
    enc = unet.init_conv_mask
    assert not enc.trainable and all(not p.requires_grad for p in enc.parameters())
    cond = fill.hash_tensor((2, 3, 32, 32), "swin.cond", 1.0).to(gpu)
    x = fill.hash_tensor((2, 3, 32, 32), "swin.train.x", 1.0).to(gpu)
    enc.train()
    a = enc(cond)
    enc.eval()
    assert all(not f.requires_grad for f in a) and all(torch.equal(p, q) for p, q in zip(a, enc(cond)))
    x1, x2 = unet(x, torch.tensor([0.3, 0.7], device=gpu), cond)
    (x1.sum() + x2.sum()).backward()
    assert all(p.grad is None for p in enc.parameters()) and unet.final_conv.weight.grad is not None
    flat = FlatParams(unet)
    assert not any(p is q for q in flat.params for p in enc.parameters())
