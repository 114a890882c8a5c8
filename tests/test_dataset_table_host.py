"""Host: which stream every driver builds for every way a data section can name a dataset.

The table below was recorded from the drivers as they stood BEFORE the dataset table of adm_amd/ddm/datasets.py existed, when each of
them spelled the selection out by hand; the table-driven drivers must reproduce it entry for entry -- the stream's class, or the
exception's type and full message.  The stream classes' constructors are replaced by recorders, so nothing is decoded or drawn and no
device is needed: the constructors' own refusals (SRBatchStream, the pair streams, ImageStream ...) are pinned by their own host tests.
"""
import itertools

import pytest

DATASETS = ("ImageDataset", "SRDataset", "SRDatasetTest", "InpaintDataset", "DUTSDataset", "SketchDataset")
CLASS_NAMES = [p + d for d in DATASETS for p in ("ddm.data.", "")] + ["synthetic", None, "nonsense"]
SYNTHETIC_OF = [None] + ["ddm.data." + d for d in DATASETS]          # None: the key is absent
COLUMNS = ("batch_stream", "first_stage_stream", "image_stream", "stream_class", "sample_cond_ldm", "sample_cond_dpm")

VAE_REFUSAL = ("NotImplementedError: data.synthetic_of {!r}: a synthetic first-stage pool is built for ddm.data.ImageDataset, "
               "ddm.data.DUTSDataset, ddm.data.SketchDataset and ddm.data.SRDataset")
DPM_REFUSAL = "NotImplementedError: data.class_name {!r}: the pixel-space conditional sampler reads ddm.data.DUTSDataset"

# class_name -> the row of COLUMNS, or {synthetic_of -> row} where synthetic_of matters.  "X/3": the driver set ``channels = 3`` on X.
IMAGE = ("SRBatchStream", "ImageFolderStream", "ImageFolderStream", "ImageFolderStream", None, DPM_REFUSAL)
SR = ("SRBatchStream", "SRBatchStream/3", "ImageStream", None, None, DPM_REFUSAL)
PLAIN = ("SRBatchStream", "ImageStream/3", "ImageStream", None, None, DPM_REFUSAL)
INPAINT = ("InpaintBatchStream", "ImageStream/3", "ImageStream", None, "ddm.data.InpaintDataset", DPM_REFUSAL)
DUTS = ("DUTSBatchStream", "DUTSMapStream", "ImageStream", "DUTSMapStream", "ddm.data.DUTSDataset", "ok")
SKETCH = ("SketchBatchStream", "SketchPhotoStream", "ImageStream", "SketchPhotoStream", "ddm.data.SketchDataset", DPM_REFUSAL)
EXPECTED = {
    "ddm.data.ImageDataset": IMAGE, "ImageDataset": IMAGE, "ddm.data.SRDataset": SR, "SRDataset": SR,
    "ddm.data.SRDatasetTest": PLAIN, "SRDatasetTest": PLAIN, "ddm.data.InpaintDataset": INPAINT, "InpaintDataset": INPAINT,
    "ddm.data.DUTSDataset": DUTS, "DUTSDataset": DUTS, "ddm.data.SketchDataset": SKETCH, "SketchDataset": SKETCH,
    None: PLAIN, "nonsense": PLAIN,
    "synthetic": {
        None: PLAIN, "ddm.data.ImageDataset": IMAGE, "ddm.data.SRDataset": SR,
        "ddm.data.SRDatasetTest": ("SRBatchStream", VAE_REFUSAL, "ImageStream", None, None, DPM_REFUSAL),
        "ddm.data.InpaintDataset": ("InpaintBatchStream", VAE_REFUSAL, "ImageStream", None, None, DPM_REFUSAL),
        # at sampling time synthetic_of selects the recipe for the sketch dataset only (sample_cond_ldm falls through to its SR
        # CondStream for the other two); sample_cond_dpm honours it
        "ddm.data.DUTSDataset": DUTS[:4] + (None, "ok"),
        "ddm.data.SketchDataset": SKETCH},
}


def observe(monkeypatch):
    """{(class_name, synthetic_of): row of COLUMNS} of the drivers as they are."""
    import sample_cond_dpm
    import sample_cond_ldm
    import train_cond_ldm
    import train_uncond_dpm
    import train_vae
    from adm_amd.ddm import image_data, inpaint_data, pair_data, sr_data
    for cls in (sr_data.SRBatchStream, inpaint_data.InpaintBatchStream, pair_data.PairBatchStream, image_data.ImageBatchStream,
                train_uncond_dpm.ImageStream):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: None)

    def built(fn, cfg):
        try:
            s = fn(cfg, 2, (32, 32), "cpu", 0)
        except Exception as e:
            return f"{type(e).__name__}: {e}"
        return type(s).__name__ + (f"/{s.__dict__['channels']}" if "channels" in s.__dict__ else "")

    def returned(fn, cfg, name=lambda r: r):
        try:
            r = fn(cfg)
        except Exception as e:
            return f"{type(e).__name__}: {e}"
        return None if r is None else name(r)

    seen = {}
    for cls, of in itertools.product(CLASS_NAMES, SYNTHETIC_OF):
        cfg = dict({"class_name": cls}, **({} if of is None else {"synthetic_of": of}))
        seen[cls, of] = (built(train_cond_ldm.batch_stream, cfg), built(train_vae.first_stage_stream, cfg),
                         built(train_uncond_dpm.image_stream, cfg), returned(image_data.stream_class, cfg, lambda c: c.__name__),
                         returned(sample_cond_ldm.sampling_dataset, cfg),
                         returned(lambda c: sample_cond_dpm.check_dataset(c) or "ok", cfg))
    return seen


def expected():
    out = {}
    for cls, of in itertools.product(CLASS_NAMES, SYNTHETIC_OF):
        row = EXPECTED[cls]
        row = row[of] if isinstance(row, dict) else row
        out[cls, of] = tuple(c.format(of if "synthetic_of" in c else cls) if isinstance(c, str) else c for c in row)
    return out


def test_every_driver_selects_what_it_selected_before_the_table(monkeypatch):
    seen, want = observe(monkeypatch), expected()
    assert len(want) == len(CLASS_NAMES) * len(SYNTHETIC_OF) == 105
    wrong = {k: dict(zip(COLUMNS, zip(seen[k], want[k]))) for k in want if seen[k] != want[k]}
    assert not wrong, wrong
