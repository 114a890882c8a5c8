#!/usr/bin/env python3
"""Golden GRADIENTS of the Swin condition encoder in train mode (the backward pass and stochastic depth).
RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).

Imports the REAL reference module unet.swin_transformer, as tools/make_golden_swin.py does: import-time placeholders for
torchvision plus FUNCTIONAL stand-ins written here for MLP, Permute and StochasticDepth.  The StochasticDepth stand-in restates
torchvision's "row" mode as the reference uses it (StochasticDepth(sd_prob, "row") around both branches of a block): in
training and with p > 0 the branch of sample b is multiplied by keep_b / (1 - p); the identity otherwise.  It is a stand-in, not
torchvision's class: its draws keep_b come from a FIXED TABLE (tests/swin_train_ref.py: KEEP_SMALL), not from a generator, so that
the restatement and the HIP module can be given the same draws.

Runs the reference's own ShiftedWindowAttention, PatchMerging and SwinTransformer in float64 and .train() mode, differentiates
loss = sum(output * hash-filled weights) with autograd, checks the restatement tests/swin_train_ref.py against it on identical
inputs, then writes tests/golden/g20_swin_train.npz (gradients sampled by swin_train_ref.sample_grad) and
tests/golden/oracle_vs_reference_report_swin_train.json.
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)


class _Meta(type):
    def __getattr__(cls, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return cls()


class _Stub(metaclass=_Meta):
    """import-time placeholder: any attribute exists; an instance applied to a function returns the function"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else self

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub()


class _StubModule(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub


for name in ["torchvision", "torchvision.ops", "torchvision.ops.misc", "torchvision.ops.stochastic_depth", "torchvision.transforms",
             "torchvision.transforms._presets", "torchvision.utils", "torchvision.models", "torchvision.models._api",
             "torchvision.models._meta", "torchvision.models._utils"]:
    m = _StubModule(name); m.__path__ = []; sys.modules[name] = m


class MLP(nn.Sequential):
    def __init__(self, in_channels, hidden_channels, activation_layer=nn.ReLU, inplace=None, dropout=0.0, **kw):
        layers, d = [], in_channels
        for h in hidden_channels[:-1]:
            layers += [nn.Linear(d, h), activation_layer(), nn.Dropout(dropout)]
            d = h
        layers += [nn.Linear(d, hidden_channels[-1]), nn.Dropout(dropout)]
        super().__init__(*layers)


class Permute(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.permute(*self.dims)


class StochasticDepth(nn.Module):
    """Functional stand-in for torchvision.ops.StochasticDepth(p, "row"): draws from DRAWS[(block, branch)] (set below)."""
    DRAWS = None          # [n_blocks, 2, B] of 0 / 1

    def __init__(self, p, mode):
        super().__init__()
        assert mode == "row"
        self.p, self.block, self.calls = float(p), None, 0

    def forward(self, x):
        branch = self.calls % 2          # a block calls it for the attention branch, then for the MLP branch
        self.calls += 1
        if not self.training or self.p == 0.0:
            return x
        keep = StochasticDepth.DRAWS[self.block, branch].to(x.dtype)
        return x * (keep / (1.0 - self.p)).view(-1, *([1] * (x.dim() - 1)))


sys.modules["torchvision.ops.misc"].MLP = MLP
sys.modules["torchvision.ops.misc"].Permute = Permute
sys.modules["torchvision.ops.stochastic_depth"].StochasticDepth = StochasticDepth
sys.modules["torchvision.utils"]._log_api_usage_once = lambda obj: None

import unet.swin_transformer as S  # noqa: E402  (the reference's)

import swin_ref as R  # noqa: E402
import swin_train_ref as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)
torch.set_default_dtype(torch.float64)
report = {"torch": torch.__version__, "cases": []}
g = {}


def check(name, got, want, tol=1e-11):
    e = float((got - want).abs().max() / (want.abs().max() + 1e-300))
    ok = e <= tol
    report["cases"].append(dict(case=name, max_rel_err=e, tol=tol, ok=bool(ok)))
    if not ok:
        print(f"BAD {name}: rel_err={e:.3e}")
    assert ok, name


# ------------------------------------------------------------------------------------------------ attention modules
for name, (B, H, W, C, heads, shift) in R.ATTN_CASES.items():
    x, sd = R.attn_case_inputs(name)
    att = S.ShiftedWindowAttention(C, [7, 7], [shift, shift], heads).train()
    p = name + "."
    att.load_state_dict({"qkv.weight": sd[p + "qkv.weight"], "qkv.bias": sd[p + "qkv.bias"],
                         "relative_position_bias_table": sd[p + "relative_position_bias_table"],
                         "proj.weight": torch.eye(C), "proj.bias": torch.zeros(C)}, strict=False)
    x = x.clone().requires_grad_(True)
    y = att(x)
    gs = torch.autograd.grad((y * T.weight_like(y, f"attn.{name}.d_out")).sum(),
                             [x, att.qkv.weight, att.qkv.bias, att.relative_position_bias_table])
    mine = T.attn_module_grads(name)
    for (k, m), r in zip(mine.items(), gs):
        check(f"attn/{name}/{k}", m, r)
        g[f"attn.{name}.{k}"] = T.sample_grad(r).numpy().copy()

# ------------------------------------------------------------------------------------------------ PatchMerging
for name, (B, H, W, C) in R.MERGE_CASES.items():
    x, sd = R.merge_case_inputs(name)
    pm = S.PatchMerging(C, nn.LayerNorm).train()
    pm.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items()})
    x = x.clone().requires_grad_(True)
    y = pm(x)
    gs = torch.autograd.grad((y * T.weight_like(y, f"merge.{name}.d_out")).sum(), [x, pm.norm.weight, pm.norm.bias, pm.reduction.weight])
    mine = T.merge_grads(name)
    for (k, m), r in zip(mine.items(), gs):
        check(f"merge/{name}/{k}", m, r)
        g[f"merge.{name}.{k}"] = T.sample_grad(r).numpy().copy()

# ------------------------------------------------------------------------------------------------ the small model, with and without drops
cfg = R.SMALL
for tag, p, keep in (("small.sd0", 0.0, None), ("small.sd5", 0.5, T.KEEP_SMALL)):
    m = S.SwinTransformer(patch_size=[4, 4], embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]),
                          window_size=[7, 7], stochastic_depth_prob=p).train()
    m.load_state_dict(R.filled_state_dict(**cfg), strict=True)
    blocks = [b for i, stage in enumerate(m.features) if i % 2 == 0 for b in stage]
    probs = T.sd_probs(cfg["depths"], p)
    for k, b in enumerate(blocks):
        b.stochastic_depth.block = k
        assert abs(b.stochastic_depth.p - probs[k]) < 1e-15, "the p_k schedule"
    StochasticDepth.DRAWS = keep
    x = R.model_input("small", R.SMALL_INPUT).requires_grad_(True)
    loss = T.model_loss(m(x), tag)
    loss.backward()
    mine = T.model_grads(cfg, R.SMALL_INPUT, "small", tag, keep, p)
    params = dict(m.named_parameters())
    assert all(params[k].grad is None for k in params if k.startswith(("norm.", "head."))), "norm / head take no part"
    for k, mg in mine.items():
        r = x.grad if k == "x" else params[k].grad
        check(f"{tag}/{k}", mg, r)
        g[f"{tag}.{k}"] = T.sample_grad(r).numpy().copy()
    g[f"{tag}.names"] = np.array(json.dumps(list(mine)))
assert len(json.loads(str(g["small.sd0.names"]))) == 118          # 117 trainable tensors and the input

np.savez_compressed(os.path.join(OUT, "g20_swin_train.npz"), **g)
report["max_rel_err"] = max(c["max_rel_err"] for c in report["cases"])
report["n_cases"] = len(report["cases"])
json.dump(report, open(os.path.join(OUT, "oracle_vs_reference_report_swin_train.json"), "w"), indent=1)
print(f"ALL OK: {report['n_cases']} cases, max rel err {report['max_rel_err']:.3e}; "
      f"g20_swin_train.npz = {os.path.getsize(os.path.join(OUT, 'g20_swin_train.npz'))} bytes")
