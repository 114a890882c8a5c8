"""Which reference dataset a ``data`` section names, and what every driver does with it: ONE table behind train_cond_ldm.py /
train_cond_dpm.py (``cond_stream``), train_vae.py and the unconditional trainers (``first_stage``) and sample_cond_ldm.py /
sample_cond_dpm.py (``sampling``).  Adding a recipe = its stream class(es) in their own module, one row of ``DATASETS`` here, and --
only if it predicts in a new way -- one function in sample_cond_ldm.FORMS.  The streams keep their own refusals; this module only
picks the class.
"""
from collections import namedtuple

from .depth_data import DEPTH_CLASSES, DepthBatchStream, DepthMapStream
from .image_data import IMAGE_CLASSES, DUTSMapStream, ImageFolderStream, SketchPhotoStream
from .inpaint_data import InpaintBatchStream
from .pair_data import DUTS_CLASSES, SKETCH_CLASSES, DUTSBatchStream, SketchBatchStream
from .sr_data import SRBatchStream

SR_CLASSES = ("ddm.data.SRDataset", "SRDataset")
INPAINT_CLASSES = ("ddm.data.InpaintDataset", "InpaintDataset")


def dataset_of(data_cfg):
    """The key of ``DATASETS`` that ``data_cfg`` stands for -- its ``class_name``, with or without ``ddm.data.``, or its ``synthetic_of``
    under ``class_name: synthetic`` -- or None."""
    data_cfg = data_cfg or {}
    cls = data_cfg.get("class_name")
    name = data_cfg.get("synthetic_of") if cls == "synthetic" else cls
    return next((c[0] for c in (IMAGE_CLASSES, SR_CLASSES, INPAINT_CLASSES, DUTS_CLASSES, SKETCH_CLASSES, DEPTH_CLASSES)
                 if name in c), None)


# What sample_cond_ldm.py does with a dataset's items:
#   form        which of sample_cond_ldm.FORMS makes the prediction
#   item        (stream, index, batch) -> (ori_size, file name or None) of the one-image test batch
#   split_test  the ValueError of a data section without ``split: test``, or None where the split is not checked
#   no_flip     construct the stream with ``augment_horizontal_flip: False``
#   one_window  the recipe's name in the NotImplementedError for sampler.crop_size != image_size, or None where windows slide
#   psnr / gray / save_masks   score against 'image'; one channel is a mode-L png; ``sampler.save_masks`` writes masks/<name>
#   synthetic   whether ``class_name: synthetic`` + ``synthetic_of`` selects this entry at sampling time
#   depth       the prediction is a depth fraction: written as a 16-bit png of round(clip(p, 0, 1) * 10000) (8 bits with
#               ``sampler.depth_png8``) and scored with adm_amd.metrics.depth against 'image' into <save_folder>/depth_metrics.json
#   saliency    the prediction is a saliency map: ``sampler.cal_saliency: True`` (off by default) scores its bytes against the resized
#               map's bytes with adm_amd.metrics.saliency into <save_folder>/saliency_metrics.json
Sampling = namedtuple("Sampling", "form item split_test no_flip one_window psnr gray save_masks synthetic depth saliency",
                      defaults=(None, None, False, None, True, False, False, False, False, False))
# every data section that selects no entry below: the super-resolution items of sample_cond_ldm.CondStream
SR_SAMPLING = Sampling("slide_x4")

Dataset = namedtuple("Dataset", "cond_stream first_stage sampling")          # None: the driver's fall-through stream refuses it
DATASETS = {
    IMAGE_CLASSES[0]: Dataset(None, ImageFolderStream, None),
    SR_CLASSES[0]: Dataset(SRBatchStream, SRBatchStream, None),          # (sampled from ddm.data.SRDatasetTest, by CondStream)
    INPAINT_CLASSES[0]: Dataset(InpaintBatchStream, None, Sampling(
        "composite", lambda s, k, b: ((s.size, s.size), s.names[k][:-4] + ".png" if s.names else None),      # reference :217: as png
        no_flip=True, one_window="in-painting", save_masks=True)),
    DUTS_CLASSES[0]: Dataset(DUTSBatchStream, DUTSMapStream, Sampling(
        "slide", lambda s, k, b: (b["ori_size"][0], b["img_name"][0][:-4] + ".png"),          # reference :215-216: the photo's name, as png
        split_test="sampling ddm.data.DUTSDataset needs data.split: test (DUTS-TE, in order, unflipped)", gray=True,
        saliency=True)),
    SKETCH_CLASSES[0]: Dataset(SketchBatchStream, SketchPhotoStream, Sampling(
        "window", lambda s, k, b: (b["ori_size"][0], b["img_name"][0]),          # the sketch's file name (= the photo's)
        split_test="sampling ddm.data.SketchDataset needs data.split: test (GT/val + Sketch/val, in order, unflipped)",
        one_window="sketch-to-image", psnr=False,
        synthetic=True)),          # reached by synthetic_of at sampling time: kept as found, not a decision (README)
    DEPTH_CLASSES[0]: Dataset(DepthBatchStream, DepthMapStream, Sampling(
        "slide", lambda s, k, b: (b["ori_size"][0], b["img_name"][0][:-4] + ".png"),          # the photo's name, as png
        split_test="sampling ddm.data.NYUDv2DepthDataset needs data.split: test (whole 426x560 frames, in order, unflipped)",
        gray=True, psnr=False, depth=True,
        synthetic=True)),          # a decision: the committed sample YAML runs without data (README)
}


def sampling_dataset(data_cfg):
    """The key of the entry whose ``sampling`` sample_cond_ldm.py follows, or None: SR_SAMPLING."""
    key = dataset_of(data_cfg)
    sampling = DATASETS[key].sampling if key else None
    if sampling is None or ((data_cfg or {}).get("class_name") == "synthetic" and not sampling.synthetic):
        return None
    return key
