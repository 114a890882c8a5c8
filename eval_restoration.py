#!/usr/bin/env python3
"""The restoration score of a folder of restored images against a folder of targets, on the HIP metrics kernel: what
sample_cond_ldm.py prints with ``sampler.cal_restoration: True``, for predictions made anywhere.

  python eval_restoration.py --pred <folder> --target <folder> [--crop-border 4] [--out_path result.json]

Both folders hold 8-bit PNG / JPG files (adm_amd.metrics.evaluate.list_images), paired by file stem; every target needs a prediction,
read as RGB.  Each pair is scored at its own size; pairs of equal size share a launch.  Nothing is resized: a prediction whose size
differs from its target's raises and names the file, as do a missing prediction and a pair too small for the shave plus the 11 x 11
SSIM window.  One process only.  The JSON keys are psnr, ssim, psnr_y, ssim_y (adm_amd/metrics/restoration.py) and images;
``--crop-border`` defaults to 0 -- x4 super-resolution tables use 4 and the Y pair, in-painting tables 0 and the RGB pair.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def find_pairs(pred_folder, target_folder):
    """[(prediction path, target path)] in the targets' order; a target without a prediction of its stem raises and names the file."""
    from adm_amd.metrics.evaluate import list_images
    preds = {}
    for path in list_images(pred_folder):
        preds.setdefault(os.path.splitext(os.path.basename(path))[0], path)
    out = []
    for target in list_images(target_folder):
        stem = os.path.splitext(os.path.basename(target))[0]
        if stem not in preds:
            raise FileNotFoundError(f"the prediction for {target} is missing: no {stem}.png / .jpg in {pred_folder}")
        out.append((preds[stem], target))
    if not out:
        raise FileNotFoundError(f"{target_folder} holds no png / jpg target")
    return out


def read_pairs(files, crop_border):
    """{(H, W): [(prediction uint8 [3,H,W], target, path)]}; a size mismatch or a pair too small raises and names the file."""
    import numpy as np
    from PIL import Image
    from adm_amd.metrics.restoration import WINDOW
    groups = {}
    for path, target in files:
        try:
            with Image.open(path) as a, Image.open(target) as b:
                p, g = np.asarray(a.convert("RGB"), dtype=np.uint8), np.asarray(b.convert("RGB"), dtype=np.uint8)
        except Exception as e:
            raise OSError(f"{path} or {target} cannot be read as an image: {e}") from e
        if p.shape != g.shape:
            raise ValueError(f"{path} is {p.shape[0]}x{p.shape[1]} but its target {target} is {g.shape[0]}x{g.shape[1]}: nothing is resized here")
        H, W = p.shape[:2]
        if H - 2 * crop_border < WINDOW or W - 2 * crop_border < WINDOW:
            raise ValueError(f"{path} is {H}x{W}: shaved by --crop-border {crop_border} it leaves {H - 2 * crop_border}x{W - 2 * crop_border}, "
                             f"smaller than the {WINDOW}x{WINDOW} SSIM window")
        groups.setdefault((H, W), []).append((p.transpose(2, 0, 1), g.transpose(2, 0, 1), path))
    return groups


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred", required=True)
    ap.add_argument("--target", required=True)
    ap.add_argument("--crop-border", type=int, default=0)
    ap.add_argument("--out_path", default=None)
    args = ap.parse_args(argv)
    if args.crop_border < 0:
        raise ValueError(f"--crop-border must be >= 0, got {args.crop_border}")
    if int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise RuntimeError("eval_restoration.py runs in one process (its score is not reduced across ranks)")
    groups = read_pairs(find_pairs(args.pred, args.target), args.crop_border)          # (before anything touches the GPU)
    import numpy as np
    import torch
    from adm_amd.metrics.restoration import RestorationScore
    if not torch.cuda.is_available():
        raise RuntimeError("eval_restoration.py runs the metrics kernel: it needs a GPU")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    score = RestorationScore(args.crop_border)
    for (H, W), items in groups.items():
        per = max(1, min(64, (1 << 26) // (3 * H * W)))          # bounded launches; the sums stay on the device
        for i in range(0, len(items), per):
            chunk = items[i:i + per]
            score.add(torch.from_numpy(np.stack([p for p, _, _ in chunk])).to(device), torch.from_numpy(np.stack([g for _, g, _ in chunk])).to(device))
    res = score.result()
    if args.out_path:
        with open(args.out_path, "w") as f:
            json.dump(res, f)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
