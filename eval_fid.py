#!/usr/bin/env python3
"""FID (and Inception score, and KID) of two image sets on the HIP InceptionV3 extractor: the counterpart of ``fidelity -f -i -k``.

  python eval_fid.py --input1 <folder|stats.npz|features.npz> --input2 <folder|stats.npz|features.npz> --weights <pth> [--isc]
                     [--batch-size 64] [--out_path result.json] [--save-stats x.npz]
                     [--kid] [--kid-subsets 100] [--kid-subset-size 1000] [--kid-degree 3] [--kid-gamma G] [--kid-coef0 1]
                     [--save-features x.npz]

A folder is its png / jpg / jpeg files sorted by name, decoded with PIL to RGB uint8.  ``--weights`` is a local copy of
torch-fidelity's ``weights-inception-2015-12-05`` state dict; nothing is fetched.  ``--save-stats`` keeps the statistics of input1
(``mu``, ``sigma``, ``n`` in float64).  The Inception score is that of input1, which must then be a folder.

``--kid`` adds the kernel Inception distance (adm_amd/metrics/kid.py; one launch of ``adm_kid_sums`` for all subsets): the defaults
are fidelity's, ``--kid-gamma`` unset means 1 / 2048, and a subset size above either image count is refused.  KID needs the features
themselves, so each input is a folder or a file written by ``--save-features``: ``--save-features a.npz`` keeps the features of
input1 (float32 ``features`` [N, 2048]), ``--save-features a.npz b.npz`` those of input2 as well.  Such a file serves FID too: its
statistics are streamed from the features.  A statistics ``.npz`` given to ``--kid`` or ``--save-features`` is an error.  The JSON keys are fidelity's: frechet_inception_distance, inception_score_mean, inception_score_std,
kernel_inception_distance_mean, kernel_inception_distance_std.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input1", required=True)
    ap.add_argument("--input2", required=True)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--isc", action="store_true")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--out_path", default=None)
    ap.add_argument("--save-stats", default=None)
    ap.add_argument("--kid", action="store_true")
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--kid-degree", type=int, default=3)
    ap.add_argument("--kid-gamma", type=float, default=None)
    ap.add_argument("--kid-coef0", type=float, default=1.0)
    ap.add_argument("--save-features", nargs="+", default=None, metavar="NPZ",
                    help="keep the features of input1 (and, with a second path, of input2)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from adm_amd.metrics import evaluate
    evaluate.check_startup(args.weights, "eval_fid.py")
    if args.isc and args.input1.lower().endswith(".npz"):
        raise ValueError("--isc needs the images of --input1, not saved statistics")
    if args.save_features and len(args.save_features) > 2:
        raise ValueError("--save-features takes one path (input1) or two (input1, input2)")
    inputs = (args.input1, args.input2)
    save = (list(args.save_features or []) + [None, None])[:2]
    keep = [args.kid or path is not None for path in save]      # per input: are its features needed?
    for src, k in zip(inputs, keep):      # refused before the extractor is built: statistics hold no features
        if k and os.path.isfile(src) and src.lower().endswith(".npz") and not evaluate.is_feature_file(src):
            evaluate.load_features(src)
    scorer = evaluate.Scorer(args.weights, isc=args.isc)

    def read(i, logits):
        if not keep[i]:
            return scorer.input_stats(inputs[i], args.batch_size, logits) + (None,)
        st, lg, feats = scorer.input_features(inputs[i], args.batch_size, logits)
        if save[i]:
            evaluate.save_features(save[i], feats)
        return st, lg, feats
    st1, logits, f1 = read(0, True)
    if args.save_stats:
        evaluate.save_stats(args.save_stats, st1)
    st2, _, f2 = read(1, False)
    kid_res = None
    if args.kid:
        from adm_amd.metrics import kid
        kid_res = kid.kid_from_features(f1, f2, subsets=args.kid_subsets, subset_size=args.kid_subset_size, degree=args.kid_degree,
                                        gamma=args.kid_gamma, coef0=args.kid_coef0)
    res = evaluate.score(st1, st2, logits, args.out_path, extra=kid_res)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
