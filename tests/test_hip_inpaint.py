"""GPU: the in-painting kernels (adm_amd/csrc/inpaint_data.hip) against the NumPy restatement tests/inpaint_ref.py, which
tests/test_inpaint_host.py pins to the reference's own run (tests/golden/g22_inpaint.npz).  No PIL, no reference import.

Everything here is a condition, not a tolerance: primitive lists, masks and the float outputs are compared for equality (the mask is
defined in integers; the floats are the host expression evaluated operation by operation).  The only tolerances are those of
test_hip_cond.py, reused for the denoiser at the recipe's widths."""
import os

import numpy as np
import pytest
import torch

import inpaint_ref as R
from oracle import fill
from sr_data_ref import hash_bytes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_inpaint.npz")
LISTS = ("rects", "verts", "nverts", "widths", "flips")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def golden_lists(g, tag, S):
    """The golden's primitive lists in the kernel's layout (rectangles clipped)."""
    raw, drawn = g[f"{tag}.raw_rects"], g[f"{tag}.rect_drawn"]
    rects = np.zeros(raw.shape, np.int32)
    for b in range(raw.shape[0]):
        for j in range(raw.shape[1]):
            if drawn[b, j]:
                rects[b, j] = R.clip_rect(*(int(v) for v in raw[b, j]), S)
    return {"rects": rects, "verts": g[f"{tag}.verts"], "nverts": g[f"{tag}.nverts"], "widths": g[f"{tag}.widths"], "flips": g[f"{tag}.flips"]}


def run_batch(gpu, images, idx, flip, prims, S):
    from adm_amd.ddm.inpaint_data import inpaint_batch
    from adm_amd.ddm.sr_data import ImagePool
    pool = ImagePool.from_uniform(torch.from_numpy(np.ascontiguousarray(images)).to(gpu), (S, S))
    out = inpaint_batch(pool, idx, flip, prims, S)
    torch.cuda.synchronize()
    return out


def check_batch(out, images, idx, flip, masks):
    image, cond, mask = (t.cpu() for t in out)
    want_image, want_cond, want_mask = R.host_batch(images, idx, flip, masks)
    wrong = int((mask != want_mask).sum())
    print(f"mask mismatches {wrong} of {mask.numel()}; image equal {torch.equal(image, want_image)}; cond equal {torch.equal(cond, want_cond)}")
    assert mask.dtype == image.dtype == cond.dtype == torch.float32 and mask.shape == want_mask.shape
    assert wrong == 0
    assert torch.equal(image, want_image) and torch.equal(cond, want_cond)


@pytest.mark.parametrize("S", [64, 256])
def test_masks_kernel_gives_the_restatements_lists(gpu, g, S):
    """The fixture's draws (B = 64, K = 4; sample 0's first three candidates and sample 1's first are empty) plus one appended sample
    whose four candidates are all empty: lists, chosen candidates and the fallback counter."""
    from adm_amd.ddm.inpaint_data import inpaint_masks
    u, z = g[f"s{S}.u"].copy(), g[f"s{S}.z"].copy()
    u, z = np.concatenate([u, u[:1]]), np.concatenate([z, z[:1]])
    u[-1, :, [R.U_NRECT_SMALL, R.U_NRECT_BIG, R.U_NSTROKE]] = 0.0
    want, fell = R.geometry_batch(u, z, S)
    assert fell == 1 and want["chosen"][0] == 3 and want["chosen"][1] == 1 and want["chosen"][-1] == 3
    assert np.array_equal(want["chosen"][:-1], g[f"s{S}.chosen"])
    counter = torch.zeros(1, dtype=torch.int32, device=gpu)
    got = inpaint_masks(torch.from_numpy(u).to(gpu), torch.from_numpy(z).to(gpu), S, counter)
    torch.cuda.synchronize()
    for k in LISTS + ("chosen",):
        a = got[k].cpu().numpy()
        print(f"{k}: {int((a != want[k]).sum())} of {a.size} entries differ")
    for k in LISTS + ("chosen",):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert int(counter) == 1
    assert not got["nverts"][-1].any() and not got["rects"][-1].any()          # the fallback: nothing drawn, an all-ones mask
    inpaint_masks(torch.from_numpy(u).to(gpu), torch.from_numpy(z).to(gpu), S, counter)
    assert int(counter) == 2          # the counter accumulates


@pytest.mark.parametrize("tag,S", [("s64", 64), ("s256", 256), ("hand64", 64), ("hand256", 256)])
def test_batch_masks_are_the_restatements(gpu, g, tag, S):
    """Every fixture sample and every hand-placed case (a vertex at (S, S), equal consecutive vertices, 18 vertices, widths 12 and
    47, rectangles clipped at each border and one outside, 3 + 1 rectangles with 7 strokes of 18 vertices, the four flip
    combinations): ori_mask equals the integer restatement, image / cond the host expression.  Images are drawn from a pool of 3,
    every second one flipped."""
    prims = golden_lists(g, tag, S)
    B = prims["rects"].shape[0]
    masks = R.raster_batch(prims, S)
    images = hash_bytes((3, S, S, 3), f"inp.pool{S}")
    idx, flip = [b % 3 for b in range(B)], [b % 2 for b in range(B)]
    out = run_batch(gpu, images, idx, flip, prims, S)
    check_batch(out, images, idx, flip, masks)
    again = run_batch(gpu, images, idx, flip, prims, S)
    assert all(torch.equal(a, b) for a, b in zip(out, again))          # two runs, bitwise equal
    assert float(out[1][out[2].expand(-1, 3, -1, -1) == 0].max()) == -1.0          # holes of cond are -1


@pytest.mark.parametrize("S,B", [(72, 3), (72, 1), (64, 1)])
def test_batch_shapes_that_are_no_tile_multiple(gpu, S, B):
    """S = 72 is no multiple of the 32 x 8 tile in x (the last tile holds 8 columns); B = 1 and B = 3; idx = the last image of the
    pool; the image flip on and off; masks from draws through both kernels, with stroke flips on and off."""
    from adm_amd.ddm.inpaint_data import inpaint_masks
    gen = torch.Generator().manual_seed(72 + B)
    u, z = torch.rand(B, R.CANDIDATES, R.NU, generator=gen), torch.randn(B, R.CANDIDATES, R.NZ, generator=gen)
    u[:, :, R.U_NSTROKE] = 0.3          # two strokes each: part of the image stays
    for b in range(B):
        u[b, :, R.U_FLIP], u[b, :, R.U_FLIP + 1] = 0.25 + 0.5 * (b % 2), 0.25 + 0.5 * ((b // 2 + 1) % 2)
    want, _ = R.geometry_batch(u.numpy(), z.numpy(), S)
    got = inpaint_masks(u.to(gpu), z.to(gpu), S)
    for k in LISTS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    images = hash_bytes((4, S, S, 3), f"inp.odd{S}")
    masks = R.raster_batch(want, S)
    assert 0 < masks.mean() < 1
    for idx, flip in (([3] * B, [1] * B), ([b % 4 for b in range(B)], [0] * B)):
        check_batch(run_batch(gpu, images, idx, flip, got, S), images, idx, flip, masks)


def test_batch_from_a_pool_of_one_image(gpu, g):
    prims = {k: v[:3] for k, v in golden_lists(g, "hand64", 64).items()}
    images = hash_bytes((1, 64, 64, 3), "inp.one")
    out = run_batch(gpu, images, [0, 0, 0], [0, 1, 0], prims, 64)
    check_batch(out, images, [0, 0, 0], [0, 1, 0], R.raster_batch(prims, 64))
    # an index past the pool is clamped to its last image, never read out of bounds
    out = run_batch(gpu, images, [5, -2, 0], [0, 1, 0], prims, 64)
    check_batch(out, images, [0, 0, 0], [0, 1, 0], R.raster_batch(prims, 64))


def test_stream(gpu, tmp_path):
    """InpaintBatchStream: keys and shapes, the same seed gives the same batches, injected draws give the restatement's batch, the
    permutation covers the pool, the image flip does not touch the mask."""
    from adm_amd.ddm.inpaint_data import InpaintBatchStream
    x = hash_bytes((5, 64, 64, 3), "inp.stream")
    np.save(tmp_path / "pool.npy", x)
    cfg = {"npy": str(tmp_path / "pool.npy"), "augment_horizontal_flip": True, "hole_range": [0, 1]}
    a, b = (InpaintBatchStream(cfg, 2, (64, 64), gpu, 7) for _ in range(2))
    for _ in range(2):
        ba, bb = next(a), next(b)
        assert list(ba) == ["image", "cond", "ori_mask"] and all(torch.equal(ba[k], bb[k]) for k in ba)
    assert tuple(ba["image"].shape) == tuple(ba["cond"].shape) == (2, 3, 64, 64) and tuple(ba["ori_mask"].shape) == (2, 1, 64, 64)
    s = InpaintBatchStream(cfg, 2, (64, 64), gpu, 8)
    draws = [s.draw() for _ in range(5)]
    assert sorted(torch.cat([d[0] for d in draws]).tolist()) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    idx, flip, u, z = s.draw()
    assert u.shape == (2, R.CANDIDATES, R.NU) and z.shape == (2, R.CANDIDATES, R.NZ) and float(u.min()) >= 0 and float(u.max()) < 1
    out = s.next_batch(idx=idx, flip=flip, u=u, z=z)
    want, _ = R.geometry_batch(u.cpu().numpy(), z.cpu().numpy(), 64)
    masks = R.raster_batch(want, 64)
    check_batch((out["image"], out["cond"], out["ori_mask"]), x, idx.tolist(), flip.tolist(), masks)
    other = s.next_batch(idx=idx, flip=1 - flip, u=u, z=z)
    assert torch.equal(other["ori_mask"], out["ori_mask"]) and torch.equal(other["image"], out["image"].flip(-1))
    assert int(s.fallbacks) == 0
    u0 = u.clone()
    u0[0, :, [R.U_NRECT_SMALL, R.U_NRECT_BIG, R.U_NSTROKE]] = 0.0          # the first sample's candidates are all empty
    out = s.next_batch(idx=idx, flip=flip, u=u0, z=z)
    assert int(s.fallbacks) == 1 and bool((out["ori_mask"][0] == 1).all()) and torch.equal(out["cond"][0], out["image"][0])
    b = next(InpaintBatchStream({"class_name": "synthetic"}, 3, (64, 64), gpu, 1))
    assert tuple(b["ori_mask"].shape) == (3, 1, 64, 64) and set(b["ori_mask"].unique().tolist()) <= {0.0, 1.0}


def test_compose(gpu):
    """mask * (cond + 1) / 2 + (1 - mask) * x on masks of {0, 1}; 2 * 3 * 37 * 29 = 6438 elements is no multiple of the 256-thread
    block.  Equal to the torch expression evaluated on the same device, and on the CPU."""
    from adm_amd.ddm.inpaint_data import inpaint_compose
    B, C, H, W = 2, 3, 37, 29
    mask = (fill.hash_tensor((B, 1, H, W), "inp.cmask", 1.0) > 0).float()
    cond, x = fill.hash_tensor((B, C, H, W), "inp.ccond", 1.0), fill.hash_tensor((B, C, H, W), "inp.cx", 1.0).abs()
    assert 0 < float(mask.mean()) < 1
    got = inpaint_compose(mask.to(gpu), cond.to(gpu), x.to(gpu))
    want = mask * ((cond + 1) * 0.5) + (1 - mask) * x
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, mask.to(gpu) * ((cond.to(gpu) + 1) * 0.5) + (1 - mask.to(gpu)) * x.to(gpu))
    assert torch.equal(got.cpu()[mask.expand(-1, C, -1, -1) == 0], x[mask.expand(-1, C, -1, -1) == 0])
    with pytest.raises(ValueError, match="do not fit"):
        inpaint_compose(mask.to(gpu)[:, :, :-1], cond.to(gpu), x.to(gpu))


def tiny_ldm(gpu):
    """The reduced in-painting model of tests/test_hip_train_inpaint.py, without its condition encoder's weights trained."""
    import yaml
    from train_uncond_dpm import Cfg, build_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.load(open(os.path.join(root, "configs/inpainting/celebahq_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    cfg["model"].update(image_size=[64, 64], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["unet"].update(dim=32, cond_feature_size=[16, 16])
    torch.manual_seed(5)
    return build_model(Cfg(cfg).model).to(gpu).eval()


def test_masked_sampling(gpu, g):
    """sample(mask=...) at 64 x 64 (16 x 16 latents): equals the compose of the unmasked sample under the same x_T; mask=None is
    what it was (the composite's holes ARE the unmasked sample, bit for bit); a feature-list cond needs cond_image."""
    from adm_amd.ddm.inpaint_data import inpaint_compose
    ldm = tiny_ldm(gpu)
    prims = {k: v[10:12] for k, v in golden_lists(g, "hand64", 64).items()}
    images = hash_bytes((2, 64, 64, 3), "inp.sample")
    _, cond, mask = run_batch(gpu, images, [0, 1], [0, 0], prims, 64)
    x_T = fill.hash_tensor((2, 3, 16, 16), "inp.xT", 1.0).to(gpu)
    plain = ldm.sample(cond=cond, x_T=x_T)
    again = ldm.sample(cond=cond, x_T=x_T, mask=None)
    assert torch.equal(plain, again) and tuple(plain.shape) == (2, 3, 64, 64)
    assert float(plain.min()) >= 0 and float(plain.max()) <= 1
    masked = ldm.sample(cond=cond, x_T=x_T, mask=mask)
    assert torch.equal(masked, inpaint_compose(mask, cond, plain))
    m3 = mask.expand(-1, 3, -1, -1)
    assert torch.equal(masked[m3 == 0], plain[m3 == 0]) and torch.equal(masked[m3 == 1], ((cond + 1) * 0.5)[m3 == 1])
    feats = list(ldm.model.init_conv_mask(cond))
    by_feats = ldm.sample(cond=feats, x_T=x_T, mask=mask, cond_image=cond)
    assert torch.equal(by_feats, inpaint_compose(mask, cond, ldm.sample(cond=feats, x_T=x_T)))
    with pytest.raises(ValueError, match="cond_image"):
        ldm.sample(cond=feats, x_T=x_T, mask=mask)


@pytest.mark.parametrize("D", [12, 24, 48, 96])
def test_mha_head_dims_of_the_recipe(gpu, D):
    """RelationNet's 8-head cross-attention at the head dims of 96 * (1, 2, 4, 8) channels, forward and the three gradients against
    float64 on the CPU; 70 keys = one full 64-key tile and a ragged one.  Bound: every output is a sum of at most D + Lk = 166
    products rounded in f32, so a relative error of the whole tensor beyond 166 * 2^-24 = 1e-5 is not rounding.  (At D = 96 the
    key-side gradient once held four 96-float arrays per thread, spilled to scratch memory and came out 17 % wrong.)"""
    from adm_amd import ops_cond as oc
    H, B, Lq, Lk = 8, 2, 4, 70
    C = H * D
    q, k, v, go = (fill.hash_tensor((B, L, C), f"mha{D}.{n}", 0.5 if n == "q" else 1.0)
                   for n, L in (("q", Lq), ("k", Lk), ("v", Lk), ("g", Lq)))
    qd, kd, vd = (t.to(gpu).requires_grad_(True) for t in (q, k, v))
    o = oc.mha(qd, kd, vd, H, 1.0)
    (o * go.to(gpu)).sum().backward()
    q6, k6, v6 = (t.double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", q6.view(B, Lq, H, D), k6.view(B, Lk, H, D))
    o6 = torch.einsum("bhij,bjhd->bihd", s.softmax(-1), v6.view(B, Lk, H, D)).reshape(B, Lq, C)
    (o6 * go.double()).sum().backward()
    err = {n: float((a.detach().cpu().double() - b.detach()).norm() / b.detach().norm())
           for n, a, b in (("o", o, o6), ("dq", qd.grad, q6.grad), ("dk", kd.grad, k6.grad), ("dv", vd.grad, v6.grad))}
    print(f"D = {D}: " + ", ".join(f"{n} {e:.2e}" for n, e in err.items()))
    assert max(err.values()) <= 166 * 2.0 ** -24


def test_recipe_widths_96_vs_oracle(gpu):
    """unet.cond_unet.Unet at the in-painting recipe's widths -- dim 96, dim_mults (1, 2, 4, 8) = 96 / 192 / 384 / 768 channels, windows
    8 / 4 / 2 / 1 on both sides -- which no other config reaches: forward and every parameter gradient against
    oracle/cond_unet_ref.py, with the bounds of test_hip_cond.test_two_decoder_variant_vs_oracle.  16 x 16 latents with the
    feature pyramid of a 64 x 64 condition: 2 x 2 windows at every level, the smallest size with more than one window."""
    import importlib

    from oracle import cond_unet_ref as O
    from parity import close
    w = [[8, 8], [4, 4], [2, 2], [1, 1]]
    cfg = O.default_cfg(dim=96, dim_mults=(1, 2, 4, 8), window_sizes1=w, window_sizes2=w, two_decoders=True)
    m = importlib.import_module("unet.cond_unet").Unet(dim=96, dim_mults=cfg["dim_mults"], cond_dim=128, cond_dim_mults=(), channels=3,
                                                      cond_in_dim=3, window_sizes1=w, window_sizes2=w, fourier_scale=16,
                                                      cfg={"cond_net": "swin", "cond_pe": False})
    sd = O.filled_state_dict(cfg)
    m.load_state_dict(sd, strict=True)
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m = m.to(gpu).eval()
    x = fill.hash_tensor((2, 3, 16, 16), "cond96.x", 1.0)
    tt = torch.tensor([0.3, 0.85])
    hm = O.cond_features(2, 64, 64)
    gx, gy = fill.hash_tensor((2, 3, 16, 16), "cond96.gx", 1.0), fill.hash_tensor((2, 3, 16, 16), "cond96.gy", 1.0)
    y1, y2 = m(x.to(gpu), tt.to(gpu), [h.to(gpu) for h in hm])
    sdo = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and k != "time_mlp.0.W" else v.clone())
           for k, v in sd.items()}
    o1, o2 = O.unet_forward(sdo, cfg, x, tt, hm)
    close(y1, o1.detach()); close(y2, o2.detach())
    ((y1 * gx.to(gpu)).sum() + (y2 * gy.to(gpu)).sum()).backward()
    ((o1 * gx).sum() + (o2 * gy).sum()).backward()
    gmax = max(float(v.grad.double().norm()) for v in sdo.values() if v.requires_grad and v.grad is not None)
    bad = []
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        want = sdo[name].grad
        err = float((p.grad.cpu().double() - want.double()).norm() / (want.double().norm() + 1e-4 * gmax))
        if err > 2e-3:
            bad.append((name, err))
    print(f"{sum(1 for _ in m.parameters())} parameter tensors, {len(bad)} beyond 2e-3")
    assert not bad, bad[:10]
