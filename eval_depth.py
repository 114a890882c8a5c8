#!/usr/bin/env python3
"""The depth score of a folder of predictions against NYUv2 ground truth, on the HIP metrics kernel: what sample_cond_ldm.py prints
for the depth recipe, for predictions made elsewhere.

  python eval_depth.py --pred <folder of 16-bit PNGs> --data_root <NYUv2 folder> [--split test] [--out_path result.json]
                       [--border_crop 41 45 601 471] [--min_depth 0.001] [--max_depth 10]

Every ``rgb_*.jpg`` of the split (adm_amd.ddm.depth_data.find_nyud_pairs) needs ``<pred>/<photo name>.png``: raw units of 1/10000 of
10 m, i.e. millimetres, as sample_cond_ldm.py writes them.  A prediction is either the boxed frame (426x560) or the whole frame, which
is then cut to the box as the ground truth is; any other size raises and names the file.  The JSON keys are abs_rel, sq_rel, rmse,
rmse_log, silog, log10, d1, d2, d3 (adm_amd/metrics/depth.py: per image, then averaged), images and skipped.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred", required=True)
    ap.add_argument("--data_root", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--out_path", default=None)
    ap.add_argument("--border_crop", type=int, nargs=4, default=None, metavar=("LEFT", "UPPER", "RIGHT", "LOWER"))
    ap.add_argument("--min_depth", type=float, default=1e-3)
    ap.add_argument("--max_depth", type=float, default=10.0)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from adm_amd.ddm.depth_data import BORDER_CROP, DEPTH_UNITS, check_box, check_frames, find_nyud_pairs, read_depth_png
    from adm_amd.metrics.depth import DepthScore
    if not torch.cuda.is_available():
        raise RuntimeError("eval_depth.py runs the metrics kernel: it needs a GPU")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    box = check_box(args.border_crop or BORDER_CROP)
    left, upper, right, lower = box
    score = DepthScore(args.min_depth, args.max_depth)
    # the fraction on the host: NumPy's float32 division is the IEEE one, as in the batch kernel
    frac = lambda a: torch.from_numpy(a.astype(np.float32) / np.float32(DEPTH_UNITS)).to(device)[None, None]
    for photo, depth in find_nyud_pairs(args.data_root, args.split):
        gt = read_depth_png(depth)
        check_frames(None, [gt.shape], box, [photo.name])
        path = os.path.join(args.pred, photo.name[:-4] + ".png")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"the prediction for {photo} is missing: {path}")
        pred = read_depth_png(path)
        if pred.shape == gt.shape:
            pred = pred[upper:lower, left:right]
        elif pred.shape != (lower - upper, right - left):
            raise ValueError(f"{path} is {pred.shape[0]}x{pred.shape[1]}: expected the boxed frame {lower - upper}x{right - left} or "
                             f"the whole frame {gt.shape[0]}x{gt.shape[1]}")
        score.add(frac(pred), frac(gt[upper:lower, left:right]))
    res = score.result()
    if args.out_path:
        with open(args.out_path, "w") as f:
            json.dump(res, f)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
