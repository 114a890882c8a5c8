"""What the drivers share: start-up checks, the sorted folder listing, uint8 decoding, and folders / batches -> statistics (and, for
KID, the features themselves) -> JSON."""
from __future__ import annotations

import json
import os
from typing import Iterable, List, Optional

import numpy as np
import torch

from .fid import KEY_FID, FeatureStats, Stats, fid_from_stats, inception_score, load_stats, save_stats
from .inception import FeatureExtractorInceptionV3

EXTENSIONS = ("png", "jpg", "jpeg")


def check_startup(weights: Optional[str], what: str) -> str:
    """The refusals every driver makes before any work: one process only, and a weights file that exists."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError(f"{what}: FID / Inception score run in one process only (WORLD_SIZE = "
                                  f"{os.environ['WORLD_SIZE']}); multi-process evaluation is not implemented")
    if not weights or not os.path.isfile(weights):
        raise FileNotFoundError(f"{what}: InceptionV3 weights file {weights!r} does not exist (nothing is fetched; copy "
                                "torch-fidelity's weights-inception-2015-12-05 state dict to this machine)")
    return weights


def list_images(folder: str) -> List[str]:
    """png / jpg / jpeg files directly in ``folder``, as real paths sorted by name (the reference's glob_samples_paths)."""
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"image folder {folder!r} does not exist")
    files = [os.path.realpath(os.path.join(folder, f)) for f in os.listdir(folder)
             if os.path.splitext(f)[1].lower().lstrip(".") in EXTENSIONS and os.path.isfile(os.path.join(folder, f))]
    return sorted(files)


def load_u8(path: str) -> torch.Tensor:
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(arr.copy()).permute(2, 0, 1)


def folder_batches(folder: str, batch_size: int) -> Iterable[torch.Tensor]:
    files = list_images(folder)
    if not files:
        raise ValueError(f"no png / jpg / jpeg images in {folder!r}")
    for i in range(0, len(files), batch_size):
        imgs = [load_u8(p) for p in files[i:i + batch_size]]
        if any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError(f"{folder!r}: images of different sizes in one batch ({sorted({tuple(im.shape) for im in imgs})})")
        yield torch.stack(imgs)


class Scorer:
    """One extractor ('2048' features, plus 'logits' when the Inception score is wanted) and the statistics of a stream of uint8
    batches."""

    def __init__(self, weights: str, isc: bool = False, device="cuda", feature: str = "2048"):
        self.device = torch.device(device)
        self.feature, self.isc = feature, isc
        self.dim = {"64": 64, "192": 192, "768": 768, "2048": 2048}[feature]
        feats = [feature] + (["logits"] if isc else [])
        self.net = FeatureExtractorInceptionV3.from_file(weights, feats).to(self.device)

    def begin(self, logits: bool = True, keep_features: bool = False) -> "Run":
        """An accumulator for batches that arrive one at a time (the samplers score each batch as they write it).  With
        ``keep_features`` it also keeps every batch's features on the device (KID needs the rows, not their moments) and ``finish()``
        returns them as a third value."""
        return Run(self, self.isc and logits, keep_features)

    def stream(self, batches: Iterable[torch.Tensor], logits: bool = True, keep_features: bool = False):
        """-> (Stats, logits [N, 1008] on the CPU or None), and the [N, D] float32 features on the device with ``keep_features``;
        ``logits=False`` lets the extractor return after the FID feature"""
        run = self.begin(logits, keep_features)
        for b in batches:
            run.add(b)
        return run.finish()

    def input_stats(self, src: str, batch_size: int, logits: bool = True):
        """``src``: an image folder, a saved ``.npz`` of statistics or one of features (neither has logits)"""
        if os.path.isfile(src) and src.lower().endswith(".npz"):
            if is_feature_file(src):
                return self.stats_from_features(load_features(src), batch_size), None
            return load_stats(src), None
        return self.stream(folder_batches(src, batch_size), logits)

    def stats_from_features(self, feats: torch.Tensor, batch_size: int) -> Stats:
        """The FID statistics of saved features, streamed through ``FeatureStats`` in chunks of ``batch_size`` rows."""
        if feats.dim() != 2 or feats.shape[1] != self.dim:
            raise ValueError(f"expected [N, {self.dim}] features, got {tuple(feats.shape)}")
        stats = FeatureStats(self.dim, self.device)
        for i in range(0, feats.shape[0], batch_size):
            stats.update(feats[i:i + batch_size].to(self.device))
        return stats.finalize()

    def input_features(self, src: str, batch_size: int, logits: bool = True):
        """``src``: an image folder or a saved ``.npz`` of features -> (Stats, logits or None, features [N, D] on the device).
        Saved statistics are refused: they hold no features."""
        if os.path.isfile(src) and src.lower().endswith(".npz"):
            feats = load_features(src).to(self.device)
            return self.stats_from_features(feats, batch_size), None, feats
        return self.stream(folder_batches(src, batch_size), logits, keep_features=True)

    def target_features(self, target_path: str, batch_size: int) -> torch.Tensor:
        """Features of the target folder on the device, computed once and cached as ``<target_path>.features.npz`` next to it (the
        statistics cache ``<target_path>.npz`` keeps its meaning; delete both when the folder's images or the weights file change)."""
        if os.path.isfile(target_path) and target_path.lower().endswith(".npz"):
            return load_features(target_path).to(self.device)
        cache = target_path.rstrip("/\\") + ".features.npz"
        if os.path.isfile(cache):
            return load_features(cache).to(self.device)
        _, _, feats = self.stream(folder_batches(target_path, batch_size), logits=False, keep_features=True)
        save_features(cache, feats)
        return feats

    def target_stats(self, target_path: str, batch_size: int) -> Stats:
        """Statistics of the target folder, computed once and cached as ``<target_path>.npz`` next to it (delete that file when the
        folder's images or the weights file change: the cache is keyed by the path alone)."""
        if os.path.isfile(target_path) and target_path.lower().endswith(".npz"):
            if is_feature_file(target_path):
                return self.stats_from_features(load_features(target_path), batch_size)
            return load_stats(target_path)
        cache = target_path.rstrip("/\\") + ".npz"
        if os.path.isfile(cache):
            return load_stats(cache)
        st, _ = self.stream(folder_batches(target_path, batch_size), logits=False)
        save_stats(cache, st)
        return st


class Run:
    def __init__(self, scorer: Scorer, want_logits: bool, keep_features: bool = False):
        self.scorer, self.want, self.keep = scorer, want_logits, keep_features
        self.stats, self.rows, self.feats = FeatureStats(scorer.dim, scorer.device), [], []

    def add(self, batch_u8: torch.Tensor) -> None:
        net = self.scorer.net
        net.features_list = [self.scorer.feature] + (["logits"] if self.want else [])
        out = net(batch_u8.to(self.scorer.device))
        self.stats.update(out[0])
        if self.keep:
            self.feats.append(out[0].detach().clone())
        if self.want:
            self.rows.append(out[1].cpu())

    def finish(self):
        res = self.stats.finalize(), (torch.cat(self.rows) if self.want else None)
        if not self.keep:
            return res
        return res + (torch.cat(self.feats) if self.feats else torch.empty(0, self.scorer.dim, device=self.scorer.device),)


def is_feature_file(path: str) -> bool:
    with np.load(path) as z:
        return "features" in z.files


def save_features(path: str, feats) -> None:
    """``feats``: [N, D] features, a tensor on any device or an array -> an ``.npz`` with the one key ``features`` (float32)."""
    a = feats.detach().cpu().numpy() if torch.is_tensor(feats) else np.asarray(feats)
    if a.ndim != 2:
        raise ValueError(f"features must be [N, D], got {a.shape}")
    with open(path, "wb") as f:            # (an open file: np.savez would append ".npz" to a bare name)
        np.savez(f, features=np.ascontiguousarray(a, dtype=np.float32))


def load_features(path: str) -> torch.Tensor:
    """-> float32 [N, D] on the CPU.  A file of ``mu`` / ``sigma`` statistics is refused by name: statistics hold no features."""
    with np.load(path) as z:
        if "features" not in z.files:
            if "mu" in z.files or "sigma" in z.files:
                raise ValueError(f"{path!r} holds FID statistics (mu / sigma), and statistics hold no features: KID needs the image "
                                 "folder or a file written by --save-features")
            raise ValueError(f"{path!r} has no 'features' array (keys: {sorted(z.files)})")
        a = z["features"]
    if a.ndim != 2:
        raise ValueError(f"{path!r}: 'features' must be [N, D], got {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def score(st1: Stats, st2: Optional[Stats], logits1, out_path: Optional[str] = None, splits: int = 10,
          extra: Optional[dict] = None) -> dict:
    """``extra``: further entries of the result (the two KID keys), written after the Inception score and the FID."""
    res = {}
    if logits1 is not None:
        res.update(inception_score(logits1, splits=splits))
    if st2 is not None:
        res[KEY_FID] = fid_from_stats(st1, st2)
    if extra:
        res.update(extra)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    return res
