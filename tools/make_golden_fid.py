#!/usr/bin/env python3
"""Golden vectors for FID / Inception score: the reference's own metrics package (torch-fidelity, vendored under metrics/ of the
reference checkout) run on the CPU.  Usage: ``python tools/make_golden_fid.py <reference checkout>``.

The reference extractor is built ONLY with ``feature_extractor_weights_path=`` a local file holding the synthetic state dict of
tests/inception_ref.py (passing None would make the class fetch its weights from the network; this tool never does).
metrics.utils imports torchvision, which is not a dependency here: a stub module in sys.modules is enough, nothing of it is called.

Writes tests/golden/g26_fid.npz (+ g26_fid_resize.npz: two channels of the one full resize result, to keep every file under
1 MiB) and tests/golden/oracle_vs_reference_report_fid.json:
  resize    the reference's float32 resize + normalise of uint8 inputs (full for 32x32, every 7th row / column + the last otherwise)
  extractor all six features in float64 for the cases of inception_ref.EXTRACT_CASES, the spatial mean of every Mixed_* output, the
            reference's float32 run and its error e32 against float64, the non-zero share of the 2048-feature
  metrics   fid_statistics_to_metric on float64 statistics of hash-filled features, the same by the eigenvalue route and the gap d;
            isc_features_to_metric on 103 x 1008 logits
  e2e       FID of two hash-filled image sets through the reference in float64 and float32 ('64' features), Inception score of 40
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.abspath(sys.argv[1])
sys.path.insert(1, REF)
for stub in ("torchvision", "torchvision.transforms", "torchvision.datasets", "torchvision.transforms.functional", "tqdm"):
    if stub not in sys.modules:
        try:
            __import__(stub)
        except ImportError:
            m = types.ModuleType(stub)
            m.__path__ = []

            def _any(name):                                       # any plain attribute is an empty class: enough for imports
                if name.startswith("__"):
                    raise AttributeError(name)
                return type(name, (), {})
            m.__getattr__ = _any
            m.tqdm = lambda it=None, **k: it
            sys.modules[stub] = m

import inception_ref as R  # noqa: E402
from adm_amd.metrics import inception as ours  # noqa: E402
from metrics.feature_extractor_inceptionv3 import FeatureExtractorInceptionV3  # noqa: E402
from metrics.interpolate_compat_tensorflow import interpolate_bilinear_2d_like_tensorflow1x  # noqa: E402
from metrics.metric_fid import fid_features_to_statistics, fid_statistics_to_metric  # noqa: E402
from metrics.metric_isc import isc_features_to_metric  # noqa: E402

torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
g, report = {}, {}

# ---- the extractor, float32 and float64 (the resize stays float32 in both: forward() casts the image to float itself)
sd = R.synthetic_state_dict(ours.state_dict_shapes())
with tempfile.TemporaryDirectory() as tmp:
    wpath = os.path.join(tmp, "synthetic_inception.pth")
    torch.save(sd, wpath)

    def build(features, double):
        m = FeatureExtractorInceptionV3("inception-v3-compat", list(features), feature_extractor_weights_path=wpath).eval()
        if double:
            m = m.double()
            m.Conv2d_1a_3x3.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
        return m
    ref32, ref64 = build(R.FEATURES, False), build(R.FEATURES, True)
    stem32, stem64 = build(("64",), False), build(("64",), True)
    log32, log64 = build(("logits",), False), build(("logits",), True)
names = list(ref32.state_dict().keys())
assert names == ours.state_dict_names(), "the package's state-dict names differ from the reference's"
g["names"] = np.array(names)

# ---- 1. resize
for H, W in R.RESIZE_SHAPES:
    img = R.images_u8((1, 3, H, W), f"fid.resize.{H}x{W}")
    out = interpolate_bilinear_2d_like_tensorflow1x(img.float(), size=(299, 299), align_corners=False, method="slow")
    out = ((out - 128) / 128).numpy()
    assert out.dtype == np.float32
    if (H, W) == R.RESIZE_SHAPES[0]:       # the full result: channel 2 here, channels 0-1 in a file of their own (1 MiB per file)
        g_full = {f"resize.{H}x{W}.c01": out[:, :2]}
        g[f"resize.{H}x{W}.c2"] = out[:, 2:]
        continue
    idx = R.sub_idx(299)
    g[f"resize.{H}x{W}"] = out[:, :, idx][:, :, :, idx]

# ---- 2. extractor
blocks = [n for n, _ in ref64.named_children() if n.startswith("Mixed_")]
report["extractor"] = {}
for tag, B, H, W in R.EXTRACT_CASES:
    img = R.images_u8((B, 3, H, W), f"fid.extract.{tag}")
    taps = {}
    hooks = [getattr(ref64, n).register_forward_hook(lambda mod, a, out, n=n: taps.__setitem__(n, out.mean((2, 3)).numpy()))
             for n in blocks]
    with torch.no_grad():
        f64, f32 = ref64(img), ref32(img)
    for h in hooks:
        h.remove()
    rep = {}
    for name, a, b in zip(R.FEATURES, f64, f32):
        a, b = a.numpy(), b.numpy()
        assert a.dtype == np.float64 and b.dtype == np.float32
        amax = float(np.abs(a).max())
        assert np.isfinite(a).all() and 1e-2 <= amax <= 1e3, (tag, name, amax)
        g[f"extract.{tag}.{name}"] = a
        g[f"extract.{tag}.{name}.f32"] = b
        rep[name] = {"max_abs": amax, "e32": float(np.abs(b.astype(np.float64) - a).max() / amax)}
    for n in blocks:
        g[f"extract.{tag}.tap.{n}"] = taps[n]
    share = float((f64[3] != 0).double().mean())
    assert share >= 0.5, f"only {share:.0%} of the 2048-feature is non-zero: change the fill"
    rep["nonzero_share_2048"] = share
    report["extractor"][tag] = rep
    print(tag, rep)

# ---- 3. metrics
report["metrics"] = {}
for D, N1, N2 in R.METRIC_CASES:
    st = []
    for k, N in enumerate((N1, N2)):
        mu, sigma = R.mean_cov64(R.metric_features(D, N, f"fid.metric.{D}.{k}"))
        st.append({"mu": mu, "sigma": sigma})
    want = fid_statistics_to_metric(st[0], st[1], False)["frechet_inception_distance"]
    # eigenvalue route: tr sqrt(S1 S2) = sum sqrt(eig(S1^1/2 S2 S1^1/2))
    lam, V = np.linalg.eigh(st[0]["sigma"])
    r1 = (V * np.sqrt(np.clip(lam, 0, None))) @ V.T
    ev = np.linalg.eigvalsh(r1 @ st[1]["sigma"] @ r1)
    d_mu = st[0]["mu"] - st[1]["mu"]
    alt = float(d_mu @ d_mu + np.trace(st[0]["sigma"]) + np.trace(st[1]["sigma"]) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())
    d = abs(alt - want) / abs(want)
    assert d <= 1e-6, f"D = {D}: the two routes differ by {d}: ill-conditioned case, replace it"
    g[f"metric.fid.{D}"] = np.array([want, alt, d])
    report["metrics"][f"fid_{D}"] = {"sqrtm": want, "eigen": alt, "d": d}
isc = isc_features_to_metric(R.isc_logits())
g["metric.isc"] = np.array([isc["inception_score_mean"], isc["inception_score_std"]])
report["metrics"]["isc"] = isc

# ---- 4. end to end
sets = R.e2e_sets()
res = {}
with torch.no_grad():
    for key, model in (("64", stem64), ("32", stem32)):
        st = []
        for s in sets:
            f = torch.cat([model(s[i:i + 50])[0] for i in range(0, s.shape[0], 50)])
            st.append(fid_features_to_statistics(f))
        res[key] = fid_statistics_to_metric(st[0], st[1], False)["frechet_inception_distance"]
    sub = sets[0][:R.E2E_ISC_N]
    isc64 = isc_features_to_metric(torch.cat([log64(sub[i:i + 10])[0] for i in range(0, R.E2E_ISC_N, 10)]), splits=R.E2E_ISC_SPLITS)
    isc32 = isc_features_to_metric(torch.cat([log32(sub[i:i + 10])[0] for i in range(0, R.E2E_ISC_N, 10)]), splits=R.E2E_ISC_SPLITS)
g["e2e.fid"] = np.array([res["64"], res["32"]])                  # want64, want32
g["e2e.isc"] = np.array([[isc64["inception_score_mean"], isc64["inception_score_std"]],
                         [isc32["inception_score_mean"], isc32["inception_score_std"]]])
report["e2e"] = {"fid_want64": res["64"], "fid_want32": res["32"], "isc_want64": isc64, "isc_want32": isc32}
print(report["metrics"], report["e2e"])

out = os.path.join(ROOT, "tests", "golden", "g26_fid.npz")
np.savez_compressed(out, **g)
out_full = os.path.join(ROOT, "tests", "golden", "g26_fid_resize.npz")
np.savez_compressed(out_full, **g_full)
with open(os.path.join(ROOT, "tests", "golden", "oracle_vs_reference_report_fid.json"), "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
for path in (out, out_full):
    assert os.path.getsize(path) < (1 << 20), path
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
