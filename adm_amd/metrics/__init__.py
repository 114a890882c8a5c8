"""FID, Inception score and KID on the HIP hot path: the InceptionV3 extractor (inception.py), the streaming float64 statistics and
the metrics (fid.py), the kernel Inception distance from kept features (kid.py: every subset's kernel sums in one launch), and the
folder evaluation the drivers share (evaluate.py); the depth-estimation score (depth.py: abs-rel, RMSE, delta ... from per-image
float64 sums made on the device); the saliency score (saliency.py: MAE, F-, E- and S-measure from one integer table per image made on
the device); the restoration score (restoration.py: PSNR and SSIM on RGB and Y from per-image sums made on the device)."""
from .fid import FeatureStats, Stats, fid_from_stats, inception_score, load_stats, save_stats  # noqa: F401
from .inception import FeatureExtractorInceptionV3  # noqa: F401
from .kid import kid_from_features, kid_indices, kid_sums, mmd_from_sums  # noqa: F401
from .saliency import SaliencyScore, metrics_from_tables, saliency_tables  # noqa: F401
from .restoration import RestorationScore, metrics_from_sums, restoration_sums  # noqa: F401
