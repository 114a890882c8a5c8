"""GPU: first-stage image batches made by adm_image_resize_batch (adm_amd/csrc/image_data.hip) against PIL's own bytes
(tests/golden/g28_image_data.npz, tools/make_golden_image_data.py), against adm_pair_resize_batch on the same bytes, and the three
streams built on it.  Everything is compared with torch.equal: the resize is integer arithmetic and the float conversion
(u8 / 255 * 2 - 1, each operation rounded) has one defined order, so there is no tolerance.  Only in-range draws and honest tables
are given to the device."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_image_data.npz")
TARGETS = [(32, 32), (48, 32), (40, 24)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def sources(g, C):
    return [g[f"c{C}.s{i}.src"] for i in range(len(g[f"c{C}.sizes"]))]


def wanted(g, C, target, idx, flip):
    H, W = target
    w = np.stack([g[f"c{C}.s{i}.t{H}x{W}" + (".flipped" if f else "")] for i, f in zip(idx, flip)])
    return torch.from_numpy(np.ascontiguousarray(w.reshape(len(idx), H, W, C)))


def check(out, u8, want):
    """out [B,C,H,W] float32 and u8 [B,H,W,C] uint8 of image_batch(..., want_u8=True); want uint8 [B,H,W,C]: PIL's bytes."""
    out, u8 = out.cpu(), u8.cpu()
    print(f"differing bytes: {int((u8 != want).sum()) if u8.shape == want.shape else 'shape'} of {want.numel()}")
    assert u8.dtype == torch.uint8 and out.dtype == torch.float32 and u8.shape == want.shape
    assert torch.equal(u8, want)
    assert torch.equal(out, ((want.float() / 255) * 2 - 1).permute(0, 3, 1, 2).contiguous())


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("C", [1, 3])
def test_golden_cases_in_one_batch(gpu, g, C, target):
    """Every source of the golden pool (C = 1: four row pitches 37..40, one pixel-wide image, a last image ending off a dword
    boundary; C = 3: up-scaling, identity, 3.2x down, a last image ending off a dword boundary) in ONE batch that mixes all the
    sizes, the first image twice, alternating flips; then the same batch with every flip inverted: both flips of every case."""
    from adm_amd.ddm.image_data import PlanePool, image_batch
    assert [tuple(t) for t in g["targets"].tolist()] == TARGETS
    src = sources(g, C)
    pool = PlanePool.from_arrays(src, target, gpu)
    assert pool.channels == C and pool.flat.numel() % 4 == 0 and sum(s.size for s in src) % 4 != 0
    idx = list(range(len(src))) + [0]
    for first in (0, 1):
        flip = [(i + first) % 2 for i in range(len(idx))]
        out, u8 = image_batch(pool, idx, flip, want_u8=True)
        assert tuple(out.shape) == (len(idx), C, *target)
        check(out, u8, wanted(g, C, target, idx, flip))
    # without the uint8 copy the floats are the same
    again, none = image_batch(pool, idx, flip)
    assert none is None and torch.equal(again, out)


@pytest.mark.parametrize("C", [1, 3])
def test_batch_of_one(gpu, g, C):
    """B = 1, the largest-ratio source (C = 3: 103x99 -> 40x24) and the last image of the pool."""
    from adm_amd.ddm.image_data import PlanePool, image_batch
    pool = PlanePool.from_arrays(sources(g, C), (40, 24), gpu)
    for i, f in ((2, 1), (pool.n - 1, 0)):
        out, u8 = image_batch(pool, [i], [f], want_u8=True)
        check(out, u8, wanted(g, C, (40, 24), [i], [f]))


@pytest.mark.parametrize("target", [(40, 24), (32, 32)])
def test_each_plane_is_the_pair_kernels_plane(gpu, g, target):
    """A PairPool and two PlanePools built from the same bytes (photos of one size, maps of another): each plane of
    adm_pair_resize_batch equals adm_image_resize_batch's, floats and bytes, for the same draws."""
    from adm_amd.ddm.image_data import PlanePool, image_batch
    from adm_amd.ddm.pair_data import PairPool, pair_batch
    photos, maps = sources(g, 3), sources(g, 1)[:4]
    pairs = PairPool.from_arrays(photos, maps, target, gpu)
    idx, flip = [3, 0, 2, 1, 2], [0, 1, 0, 1, 1]
    rgb, gray, rgb_u8, gray_u8 = pair_batch(pairs, idx, flip, want_u8=True)
    a, a_u8 = image_batch(PlanePool.from_arrays(photos, target, gpu), idx, flip, want_u8=True)
    b, b_u8 = image_batch(PlanePool.from_arrays(maps, target, gpu), idx, flip, want_u8=True)
    assert torch.equal(a, rgb) and torch.equal(a_u8, rgb_u8)
    assert torch.equal(b, gray) and torch.equal(b_u8.squeeze(-1), gray_u8)


def _tree(tmp_path, g):
    """The three datasets in one tmp folder, written as png (lossless): the golden sources.  DUTS photos and the sketches are
    stubs that no decoder could read."""
    from PIL import Image
    c1, c3 = sources(g, 1), sources(g, 3)
    folder = tmp_path / "folder"
    folder.mkdir()
    for i, a in enumerate(c3):
        Image.fromarray(a).save(folder / f"f{i}.png")
    duts = tmp_path / "duts" / "DUTS-TR"
    (duts / "DUTS-TR-Image").mkdir(parents=True), (duts / "DUTS-TR-Mask").mkdir(parents=True)
    for i, a in enumerate(c1):
        (duts / "DUTS-TR-Image" / f"d{i}.jpg").write_bytes(b"a photo that cannot be decoded")
        Image.fromarray(a).save(duts / "DUTS-TR-Mask" / f"d{i}.png")
    sk = tmp_path / "sketch"
    (sk / "GT" / "train" / "cat").mkdir(parents=True), (sk / "Sketch" / "train" / "cat").mkdir(parents=True)
    for i, a in enumerate(c3):
        Image.fromarray(a).save(sk / "GT" / "train" / "cat" / f"s{i}.png")
        (sk / "Sketch" / "train" / "cat" / f"s{i}.png").write_bytes(b"a sketch that cannot be decoded")
    return {"image": ({"class_name": "ddm.data.ImageDataset", "img_folder": str(folder)}, 3),
            "duts": ({"class_name": "ddm.data.DUTSDataset", "data_root": str(tmp_path / "duts"), "split": "train"}, 1),
            "sketch": ({"class_name": "ddm.data.SketchDataset", "data_root": str(tmp_path / "sketch"), "split": "train"}, 3)}


def test_streams(gpu, g, tmp_path, monkeypatch):
    from PIL import Image
    from adm_amd.ddm import image_data as I
    trees = _tree(tmp_path, g)
    classes = {"image": I.ImageFolderStream, "duts": I.DUTSMapStream, "sketch": I.SketchPhotoStream}
    # DUTSMapStream never opens a photo (nor SketchPhotoStream a sketch): every file PIL is asked to open is recorded
    opened, real_open = [], Image.open
    monkeypatch.setattr(Image, "open", lambda p, *a, **k: (opened.append(str(p)), real_open(p, *a, **k))[1])
    for kind, (cfg, C) in trees.items():
        cfg = dict(cfg, augment_horizontal_flip=True)
        a, b = classes[kind](cfg, 2, (32, 32), gpu, 7), classes[kind](cfg, 2, (32, 32), gpu, 7)
        n = a.pool.n
        assert a.channels == C and n == len(g[f"c{C}.sizes"])
        for _ in range(3):          # the same seed gives the same batches
            ba, bb = next(a), next(b)
            assert list(ba) == ["image"] and torch.equal(ba["image"], bb["image"])
        assert tuple(ba["image"].shape) == (2, C, 32, 32) and ba["image"].dtype == torch.float32
        assert float(ba["image"].min()) >= -1 and float(ba["image"].max()) <= 1
        # one epoch visits every image once: two epochs in full batches of 2, continued across the boundary
        s = classes[kind](cfg, 2, (32, 32), gpu, 8)
        draws = [s.draw() for _ in range(n)]
        idx = torch.cat([d[0] for d in draws]).cpu()
        assert sorted(idx.tolist()) == sorted(2 * list(range(n))) and sorted(idx[:n].tolist()) == list(range(n))
        assert idx.dtype == torch.int32 and set(torch.cat([d[1] for d in draws]).cpu().tolist()) <= {0, 1}
        # a drawn batch is PIL's bytes of its draws (the files are lossless, so the golden outputs are the expectation)
        i, f = s.draw()
        out = s.next_batch(idx=i, flip=f, want_u8=True)
        check(out["image"], out["image_u8"], wanted(g, C, (32, 32), i.cpu().tolist(), f.cpu().tolist()))
        out = s.next_batch(idx=[1, 1], flip=[1, 0], want_u8=True)          # injected draws are honoured
        check(out["image"], out["image_u8"], wanted(g, C, (32, 32), [1, 1], [1, 0]))
    assert opened and not [p for p in opened if p.endswith(".jpg") or os.sep + "Sketch" + os.sep in p], opened
    assert any("DUTS-TR-Mask" in p for p in opened)
    # the class's own flip default is off: no draw is consumed and nothing is mirrored
    nf = I.ImageFolderStream(trees["image"][0], 4, (32, 32), gpu, 9)
    assert int(torch.cat([nf.draw()[1] for _ in range(3)]).sum()) == 0


def test_synthetic_stream(gpu):
    """The synthetic pool runs the same kernel: its bytes, read back, resize on the CPU (PIL) to what the batch holds."""
    from PIL import Image
    from adm_amd.ddm.image_data import DUTSMapStream
    cfg = {"class_name": "synthetic", "synthetic_of": "ddm.data.DUTSDataset", "augment_horizontal_flip": True}
    s = DUTSMapStream(cfg, 4, (48, 64), gpu, 3)
    hw = s.pool.hw_host
    assert (hw[:, 0] < 48).any() and (hw[:, 0] > 48).any() and (hw[:, 1] < 64).any() and (hw[:, 1] > 64).any()
    i, f = s.draw()
    out = s.next_batch(idx=i, flip=f, want_u8=True)
    flat, want = s.pool.flat.cpu().numpy(), []
    for k in range(4):
        n = int(i[k])
        h, w = (int(v) for v in hw[n])
        o = int(s.pool.off[n])
        im = Image.fromarray(flat[o:o + h * w].reshape(h, w)).resize((64, 48), Image.BILINEAR)
        want.append(np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT) if int(f[k]) else im))
    check(out["image"], out["image_u8"], torch.from_numpy(np.stack(want)[..., None].copy()))
    sized = DUTSMapStream(dict(cfg, synthetic_sizes=[[20, 30], [50, 40]]), 2, (32, 32), gpu, 3)
    assert sized.pool.hw_host.tolist() == [[20, 30], [50, 40]] and tuple(next(sized)["image"].shape) == (2, 1, 32, 32)
