#!/usr/bin/env python3
"""FID (and Inception score) of two image sets on the HIP InceptionV3 extractor: the counterpart of ``fidelity -f -i``.

  python eval_fid.py --input1 <folder|stats.npz> --input2 <folder|stats.npz> --weights <pth> [--isc] [--batch-size 64]
                     [--out_path result.json] [--save-stats x.npz]

A folder is its png / jpg / jpeg files sorted by name, decoded with PIL to RGB uint8.  ``--weights`` is a local copy of
torch-fidelity's ``weights-inception-2015-12-05`` state dict; nothing is fetched.  ``--save-stats`` keeps the statistics of input1
(``mu``, ``sigma``, ``n`` in float64).  The Inception score is that of input1, which must then be a folder.  The JSON keys are
fidelity's: frechet_inception_distance, inception_score_mean, inception_score_std.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input1", required=True)
    ap.add_argument("--input2", required=True)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--isc", action="store_true")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--out_path", default=None)
    ap.add_argument("--save-stats", default=None)
    args = ap.parse_args(argv)
    from adm_amd.metrics import evaluate
    evaluate.check_startup(args.weights, "eval_fid.py")
    if args.isc and args.input1.lower().endswith(".npz"):
        raise ValueError("--isc needs the images of --input1, not saved statistics")
    scorer = evaluate.Scorer(args.weights, isc=args.isc)
    st1, logits = scorer.input_stats(args.input1, args.batch_size)
    if args.save_stats:
        evaluate.save_stats(args.save_stats, st1)
    st2, _ = scorer.input_stats(args.input2, args.batch_size, logits=False)
    res = evaluate.score(st1, st2, logits, args.out_path)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
