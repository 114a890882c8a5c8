#!/usr/bin/env python3
"""The saliency score of a folder of predictions against DUTS ground truth, on the HIP metrics kernel: what sample_cond_ldm.py /
sample_cond_dpm.py print with ``sampler.cal_saliency: True``, at the published protocol's resolution, for predictions made anywhere.

  python eval_saliency.py --pred <folder of 8-bit PNGs> --data_root <DUTS folder> [--split test] [--no-normalize] [--out_path result.json]

Every photo of the split (adm_amd.ddm.pair_data.find_duts_pairs) needs ``<pred>/<photo name>.png``, read as mode L; a missing one
raises and names the file.  The score is taken at the MAP's own resolution: a prediction of another size -- the samplers write the
model's -- is resized to its map's size with PIL's antialiased bilinear filter on the byte-exact resampling kernel
(adm_amd.ddm.image_data.PlanePool / image_batch), one pool and one launch per (prediction size, map size) pair, so the bytes scored
are those of ``Image.resize(map size, BILINEAR)``.  A size the resampler refuses (a ratio above about 7 per axis) raises and names the
file.  The JSON keys are mae, max_f, mean_f, adp_f, s_measure, max_e, mean_e, adp_e (adm_amd/metrics/saliency.py) and images.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def find_predictions(pred_folder, data_root, split):
    """[(prediction path, map path)] in ``find_duts_pairs``' order; a missing prediction raises and names the file."""
    from adm_amd.ddm.pair_data import find_duts_pairs
    out = []
    for photo, gt in find_duts_pairs(data_root, split):
        path = os.path.join(pred_folder, photo.name[:-4] + ".png")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"the prediction for {photo} is missing: {path}")
        out.append((path, gt))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred", required=True)
    ap.add_argument("--data_root", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--no-normalize", action="store_true", help="score the bytes / 255 as they are (default: stretched to [0, 1] per image)")
    ap.add_argument("--out_path", default=None)
    args = ap.parse_args(argv)
    files = find_predictions(args.pred, args.data_root, args.split)          # (before anything touches the GPU)
    import numpy as np
    import torch
    from PIL import Image
    from adm_amd.ddm.image_data import PlanePool, image_batch
    from adm_amd.metrics.saliency import SaliencyScore
    if not torch.cuda.is_available():
        raise RuntimeError("eval_saliency.py runs the metrics kernel: it needs a GPU")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    groups = {}          # (prediction size, map size) -> [(prediction, map, path)]
    for path, gt in files:
        try:
            p, m = np.asarray(Image.open(path).convert("L"), dtype=np.uint8), np.asarray(Image.open(gt).convert("L"), dtype=np.uint8)
        except Exception as e:
            raise OSError(f"{path} or {gt} cannot be read as an image: {e}") from e
        groups.setdefault((p.shape, m.shape), []).append((p, m, path))
    score = SaliencyScore(not args.no_normalize)
    for (p_hw, m_hw), items in groups.items():
        maps = torch.from_numpy(np.stack([m for _, m, _ in items])).to(device)
        preds = pool = None
        if p_hw == m_hw:
            preds = torch.from_numpy(np.stack([p for p, _, _ in items])).to(device)
        else:
            try:
                pool = PlanePool.from_arrays([p for p, _, _ in items], m_hw, device, [path for _, _, path in items])
            except ValueError as e:
                raise ValueError(f"{items[0][2]} ({p_hw[0]}x{p_hw[1]}) cannot be resized to its map's {m_hw[0]}x{m_hw[1]}: {e}") from e
        for i in range(0, len(items), 64):          # bounded launches; the tables stay on the device
            k = min(64, len(items) - i)
            chunk = preds[i:i + k] if pool is None else image_batch(pool, list(range(i, i + k)), [0] * k, want_u8=True)[1][..., 0]
            score.add(chunk.contiguous(), maps[i:i + k])
    res = score.result()
    if args.out_path:
        with open(args.out_path, "w") as f:
            json.dump(res, f)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
