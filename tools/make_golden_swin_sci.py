#!/usr/bin/env python3
"""Golden vectors of the SINGLE-CHANNEL Swin condition encoder (``single_channel_cond: True``, the sketch-to-image recipe).
RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).

Imports the REAL reference module unet.swin_transformer_for_sci with the torchvision stand-ins of tools/make_golden_swin.py and
tools/make_golden_swin_train.py (import-time placeholders plus FUNCTIONAL stand-ins for MLP, Permute and StochasticDepth in "row"
mode with draws from a fixed table).  Runs its SwinTransformer in float64 on hash-filled weights (tests/swin_sci_ref.py: the fill
of tests/swin_ref.py with a [E, 1, 4, 4] stem), checks the restatement tests/swin_sci_ref.py against it on identical inputs, then
writes tests/golden/g25_swin_sci.npz and tests/golden/oracle_vs_reference_report_swin_sci.json:
  * the stem (first_coonv: conv + Permute + LayerNorm) of the fused kernel's forward cases, three input contents each;
  * the small model on a (2, 1, 72, 88) input and Swin-B on (1, 1, 64, 64), all four stages;
  * the train-mode gradients of first_coonv.* through the small model, without and with scripted stochastic-depth draws.
Outputs are sampled by swin_ref.sample / swin_train_ref.sample_grad so the file stays small.
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

import unet.swin_transformer_for_sci as S  # noqa: E402  (the reference's)

import swin_ref as R  # noqa: E402
import swin_sci_ref as C  # noqa: E402
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
    print(f"{'OK ' if ok else 'BAD'} {name}: rel_err={e:.3e}")
    assert ok, name


def build(cfg, p=0.0):
    return S.SwinTransformer(patch_size=[4, 4], embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]),
                             num_heads=list(cfg["num_heads"]), window_size=[7, 7], stochastic_depth_prob=p)


# ------------------------------------------------------------------------------------------------ the stem alone
for name, (B, H, W, E) in C.STEM_CASES.items():
    m = build(dict(embed_dim=E, depths=(2, 2, 2, 2), num_heads=tuple(E // 32 * 2 ** i for i in range(4)))).eval()
    assert tuple(m.first_coonv[0].weight.shape) == (E, 1, 4, 4), "the one-channel patch embedding"
    sd = C.stem_params(E)
    m.first_coonv.load_state_dict({k[len("first_coonv."):]: v for k, v in sd.items()}, strict=True)
    for content in C.STEM_CONTENTS:
        x = C.stem_input(name, content)
        with torch.no_grad():
            y = m.first_coonv(x)
        assert tuple(y.shape) == (B, H // 4, W // 4, E)
        check(f"stem/{name}/{content}", C.stem(sd, x), y)
        g[f"stem.{name}.{content}"] = R.sample(y).numpy().copy()


# ------------------------------------------------------------------------------------------------ whole encoders
def run_model(tag, cfg, name, shape):
    shapes = C.param_shapes(**cfg)
    sd = C.filled_state_dict(**cfg)
    m = build(cfg).eval()
    ref = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert ref == [(k, tuple(s)) for k, s in shapes.items()], "state_dict names / shapes / order"
    m.load_state_dict(sd, strict=True)
    x = C.model_input(name, shape)
    with torch.no_grad():
        ys = m(x)
    os_ = C.forward(sd, x, cfg["depths"], cfg["num_heads"])
    g[f"{name}.shapes"] = np.array([list(y.shape) for y in ys])
    for i, (y, o) in enumerate(zip(ys, os_)):
        check(f"{tag}/{name}/stage{i}", o, y)
        g[f"{name}.stage{i}"] = R.sample(y).numpy().copy()
    g[f"{tag}.keys"] = np.array(json.dumps([[k, list(s)] for k, s in shapes.items()]))


run_model("small", R.SMALL, "small", C.SMALL_INPUT)
run_model("swin_b", R.SWIN_B, "b64", C.SWIN_B_INPUT)

# ------------------------------------------------------------------------------------------------ train-mode gradients of the stem
cfg = R.SMALL
for tag, p, keep in C.TRAIN_TAGS:
    m = build(cfg, p).train()
    m.load_state_dict(C.filled_state_dict(**cfg), strict=True)
    blocks = [b for i, stage in enumerate(m.features) if i % 2 == 0 for b in stage]
    probs = T.sd_probs(cfg["depths"], p)
    for k, b in enumerate(blocks):
        b.stochastic_depth.block = k
        assert abs(b.stochastic_depth.p - probs[k]) < 1e-15, "the p_k schedule"
    StochasticDepth.DRAWS = keep
    T.model_loss(m(C.model_input("small", C.SMALL_INPUT)), tag).backward()
    params = dict(m.named_parameters())
    for k, mg in C.stem_grads(cfg, C.SMALL_INPUT, "small", tag, keep, p).items():
        check(f"{tag}/{k}", mg, params[k].grad)
        g[f"{tag}.{k}"] = T.sample_grad(params[k].grad).numpy().copy()

np.savez_compressed(os.path.join(OUT, "g25_swin_sci.npz"), **g)
report["max_rel_err"] = max(c["max_rel_err"] for c in report["cases"])
report["n_cases"] = len(report["cases"])
json.dump(report, open(os.path.join(OUT, "oracle_vs_reference_report_swin_sci.json"), "w"), indent=1)
print(f"ALL OK: {report['n_cases']} cases, max rel err {report['max_rel_err']:.3e}; "
      f"g25_swin_sci.npz = {os.path.getsize(os.path.join(OUT, 'g25_swin_sci.npz'))} bytes")
