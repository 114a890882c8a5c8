#!/usr/bin/env python3
"""Golden vectors of the Swin condition encoder (the `init_conv_mask` of the conditional denoisers).
RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).

Imports the REAL reference module unet.swin_transformer.  Its torchvision imports are satisfied by import-time placeholders,
as in tools/make_golden_cond.py, plus three FUNCTIONAL stand-ins written here for the torchvision pieces the module tree is
made of: MLP = Sequential(Linear, GELU, Dropout, Linear, Dropout) (state_dict keys 0 and 3), Permute, and StochasticDepth as
the identity of eval mode.  With those the reference's own SwinTransformer, PatchMerging and shifted_window_attention run,
in float64, on hash-filled weights (tests/swin_ref.py holds the fill rule; weights are not stored).

Checks the restatement tests/swin_ref.py against the reference on identical inputs, then writes tests/golden/g19_swin.npz
(float64 outputs, sampled by swin_ref.sample, and the state_dict key / shape lists) and
tests/golden/oracle_vs_reference_report_swin.json.

A fresh reference module is built for every shape: the reference switches the shift off by writing into the module's
shift_size list, which would otherwise carry over from one shape to the next.
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
    def __init__(self, p, mode):
        super().__init__()

    def forward(self, x):
        return x


sys.modules["torchvision.ops.misc"].MLP = MLP
sys.modules["torchvision.ops.misc"].Permute = Permute
sys.modules["torchvision.ops.stochastic_depth"].StochasticDepth = StochasticDepth
sys.modules["torchvision.utils"]._log_api_usage_once = lambda obj: None

import unet.swin_transformer as S  # noqa: E402  (the reference's)

import swin_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)
torch.set_default_dtype(torch.float64)
report = {"torch": torch.__version__, "cases": []}
g = {}


def check(name, got, want, tol=1e-12):
    e = float((got - want).abs().max() / (want.abs().max() + 1e-300))
    ok = e <= tol
    report["cases"].append(dict(case=name, max_rel_err=e, tol=tol, ok=bool(ok)))
    print(f"{'OK ' if ok else 'BAD'} {name}: rel_err={e:.3e}")
    assert ok, name


# ------------------------------------------------------------------------------------------------ attention alone
for name, (B, H, W, C, heads, shift) in R.ATTN_CASES.items():
    x, sd = R.attn_case_inputs(name)
    att = S.ShiftedWindowAttention(C, [7, 7], [shift, shift], heads).eval()
    p = name + "."
    msg = att.load_state_dict({"qkv.weight": sd[p + "qkv.weight"], "qkv.bias": sd[p + "qkv.bias"],
                               "relative_position_bias_table": sd[p + "relative_position_bias_table"],
                               "proj.weight": torch.eye(C), "proj.bias": torch.zeros(C)}, strict=False)
    assert msg.missing_keys == ["relative_position_index"] and not msg.unexpected_keys, msg
    assert torch.equal(att.relative_position_index, R.relative_position_index()), "relative_position_index formula"
    with torch.no_grad():
        y = att(x)
    check(f"attn/{name}", R.attn_core(*R.attn_case_core(name)), y)
    g[f"attn.{name}"] = R.sample(y).numpy().copy()

# ------------------------------------------------------------------------------------------------ PatchMerging
for name, (B, H, W, C) in R.MERGE_CASES.items():
    x, sd = R.merge_case_inputs(name)
    pm = S.PatchMerging(C, nn.LayerNorm).eval()
    pm.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items()})
    seen = {}
    pm.norm.register_forward_hook(lambda mod, i, o: seen.__setitem__("ln", o.detach().clone()))
    with torch.no_grad():
        y = pm(x)
    check(f"merge/{name}/ln", R.merge_ln(x, sd[name + ".norm.weight"], sd[name + ".norm.bias"]), seen["ln"])
    check(f"merge/{name}/out", R.patch_merging(sd, name + ".", x), y)
    g[f"merge.{name}.ln"] = R.sample(seen["ln"]).numpy().copy()
    g[f"merge.{name}.out"] = R.sample(y).numpy().copy()


# ------------------------------------------------------------------------------------------------ whole encoders
def run_model(tag, cfg, inputs):
    shapes = R.param_shapes(**cfg)
    sd = R.filled_state_dict(**cfg)
    for name, shape in inputs.items():
        m = S.SwinTransformer(patch_size=[4, 4], embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]),
                              num_heads=list(cfg["num_heads"]), window_size=[7, 7]).eval()      # fresh per shape
        ref = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        assert ref == [(k, tuple(s)) for k, s in shapes.items()], "state_dict names / shapes / order"
        m.load_state_dict(sd, strict=True)
        x = R.model_input(name, shape)
        with torch.no_grad():
            ys = m(x)
        os_ = R.forward(sd, x, cfg["depths"], cfg["num_heads"])
        g[f"{name}.shapes"] = np.array([list(y.shape) for y in ys])
        for i, (y, o) in enumerate(zip(ys, os_)):
            check(f"{tag}/{name}/stage{i}", o, y, 1e-11)
            g[f"{name}.stage{i}"] = R.sample(y).numpy().copy()
    g[f"{tag}.keys"] = np.array(json.dumps([[k, list(s)] for k, s in shapes.items()]))


run_model("small", R.SMALL, {"small": R.SMALL_INPUT})
run_model("swin_b", R.SWIN_B, R.SWIN_B_INPUTS)
assert len(json.loads(str(g["small.keys"]))) == 129

np.savez_compressed(os.path.join(OUT, "g19_swin.npz"), **g)
report["max_rel_err"] = max(c["max_rel_err"] for c in report["cases"])
report["n_cases"] = len(report["cases"])
json.dump(report, open(os.path.join(OUT, "oracle_vs_reference_report_swin.json"), "w"), indent=1)
print(f"ALL OK: {report['n_cases']} cases, max rel err {report['max_rel_err']:.3e}; "
      f"g19_swin.npz = {os.path.getsize(os.path.join(OUT, 'g19_swin.npz'))} bytes")
