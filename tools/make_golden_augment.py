"""Records tests/golden/augment.npz: what the upstream reference's training loader (datasets/voc_fusion3.py VOC12SegDataset with
datasets/imutils.py) yields for a few tiny frames, together with the random draws it made.  Generator only - needs a checkout
of the reference and PIL, which the tests do not:

    python tools/make_golden_augment.py --reference DIR

The reference's modules are imported by path and its real `__getitem__` is called.  Stand-ins serve for what it imports and this
path does not need (imageio: a PIL read; torchvision, mmcv: empty modules).  The saturation and hue steps of its jitter object
are set to the identity (they need OpenCV through mmcv; segmif_amd.data leaves them out).  `random` and `numpy.random` are
wrapped only to RECORD the draws; which coins fall which way is steered by choosing the seed, and the ratio by the data set's
own rescale_range argument.  The fixture holds arrays only, no program text:

    frames   ir, mask, label (F, 60, 80), vis (F, 60, 80, 3) uint8
    samples  frame index, nw, nh, flip, bright_on, beta, contrast_on, alpha, pad_h, pad_w, cand (10, 2; the candidates actually
             drawn, the last one repeated up to ten), drawn (how many were), box (2) and the four outputs of the loader
"""
import argparse
import importlib.util
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CROP = 60, 80, 64


def load_reference_loader(ref_root):
    from PIL import Image
    folder = os.path.join(ref_root, "datasets")
    if not os.path.isfile(os.path.join(folder, "voc_fusion3.py")):
        raise RuntimeError(f"{folder}/voc_fusion3.py not found: pass the reference checkout with --reference")
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.array(Image.open(path))
    for name, mod in (("imageio", imageio), ("torchvision", types.ModuleType("torchvision")), ("mmcv", types.ModuleType("mmcv"))):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                sys.modules[name] = mod
    sys.dont_write_bytecode = True
    pkg = types.ModuleType("_segmif_ref_datasets")
    pkg.__path__ = [folder]
    sys.modules[pkg.__name__] = pkg
    mods = {}
    for sub in ("imutils", "voc_fusion3"):
        spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.{sub}", os.path.join(folder, sub + ".py"))
        mods[sub] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[sub]
        spec.loader.exec_module(mods[sub])
    return mods["voc_fusion3"], mods["imutils"]


class Recorder:
    """Wraps the generator functions the loader calls; every call goes through to the real one."""

    def __init__(self):
        self.log = []
        self._saved = []

    def __enter__(self):
        for owner, tag, names in ((random, "py", ("uniform", "random", "randrange")), (np.random, "np", ("randint",))):
            for n in names:
                real = getattr(owner, n)
                self._saved.append((owner, n, real))

                def wrapped(*a, _real=real, _key=f"{tag}.{n}", **k):
                    v = _real(*a, **k)
                    self.log.append((_key, a, v))
                    return v
                setattr(owner, n, wrapped)
        return self

    def __exit__(self, *exc):
        for owner, n, real in self._saved:
            setattr(owner, n, real)
        return False


def params_from_log(log, h, w):
    """The loader's draws in its own order: ratio, flip, brightness coin [beta], mode coin, contrast coin [alpha] (saturation and
    hue are the identity and draw nothing), H_pad, W_pad, then (H_start, W_start) until a window is accepted."""
    py = [e for e in log if e[0].startswith("py.")]
    coins = [e[2] for e in log if e[0] == "np.randint"]
    assert len(coins) == 5 and py[0][0] == "py.uniform" and py[1][0] == "py.random", log
    ratio = py[0][2]
    p = {"ratio": ratio, "nw": int(ratio * w), "nh": int(ratio * h), "flip": py[1][2] > 0.5, "bright_on": bool(coins[0]),
         "contrast_on": bool(coins[2]), "beta": 0.0, "alpha": 1.0, "pad_h": int(coins[3]), "pad_w": int(coins[4])}
    rest = py[2:]
    if p["bright_on"]:
        assert rest[0][0] == "py.uniform" and rest[0][1] == (-32, 32)
        p["beta"] = rest.pop(0)[2]
    if p["contrast_on"]:
        assert rest[0][0] == "py.uniform" and rest[0][1] == (0.5, 1.5)
        p["alpha"] = rest.pop(0)[2]
    assert rest and all(e[0] == "py.randrange" for e in rest) and len(rest) % 2 == 0
    cand = [(rest[i][2], rest[i + 1][2]) for i in range(0, len(rest), 2)]
    p["drawn"] = len(cand)
    p["cand"] = cand + [cand[-1]] * (10 - len(cand))
    return p


def make_frames():
    """Four tiny frames: smooth images that reach 0 and 255 (so that a brightness shift clips), and four kinds of label map."""
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = {"ir": [], "vis": [], "mask": [], "label": []}
    labels = []
    many = (yy // 12) * 3 + (xx // 20) % 3                     # a grid of blocks, classes 0..8 and a strip of 255
    many = (many % 9).astype(np.uint8)
    many[:, 76:] = 255
    labels.append(many)
    lop = np.full((H, W), 1, dtype=np.uint8)                   # mostly class 1, the right quarter a checker of 2..5
    lop[:, 58:] = (2 + ((yy // 6 + xx // 6) % 4))[:, 58:]
    labels.append(lop)
    labels.append(np.full((H, W), 3, dtype=np.uint8))          # one class
    labels.append(np.full((H, W), 255, dtype=np.uint8))        # nothing labelled
    for f, lab in enumerate(labels):
        base = 127.5 + 140.0 * np.sin(xx / (7.0 + f) + f) * np.cos(yy / (5.0 + f))
        vis = np.stack([base + 30 * np.sin((xx + yy) / 9.0 + c) for c in range(3)], axis=2) + rng.normal(0, 6, (H, W, 3))
        ir = 255.0 - base + rng.normal(0, 6, (H, W))
        frames["vis"].append(np.clip(vis, 0, 255).astype(np.uint8))
        frames["ir"].append(np.clip(ir, 0, 255).astype(np.uint8))
        frames["mask"].append(np.where((xx // 10 + yy // 10) % 2 == 0, np.clip(base, 0, 255), 0).astype(np.uint8))
        frames["label"].append(lab)
    return {k: np.stack(v) for k, v in frames.items()}


# (frame, rescale_range, what the draws must show) - the seed is searched until they do
WANTED = [
    (0, [0.5, 0.5], lambda p: p["flip"] and p["bright_on"] and not p["contrast_on"]),                       # padded in both axes
    (0, [2.0, 2.0], lambda p: not p["flip"] and p["contrast_on"] and not p["bright_on"] and p["alpha"] > 1.3),  # no padding
    (0, [0.85, 0.95], lambda p: p["nh"] < CROP <= p["nw"] and not p["bright_on"] and not p["contrast_on"]),  # padded in one axis
    (0, [1.2, 1.4], lambda p: p["bright_on"] and p["beta"] > 25 and p["contrast_on"] and p["flip"]),         # clips at 255
    (0, [1.2, 1.4], lambda p: p["bright_on"] and p["beta"] < -25 and not p["contrast_on"]),                  # clips at 0
    (1, [2.0, 2.0], lambda p: 3 <= p["drawn"] <= 9),                                                         # first candidates rejected
    (2, [1.5, 1.5], lambda p: p["drawn"] == 10 and len(set(p["cand"])) > 3),                                 # uniform label: last kept
    (3, [1.0, 1.0], lambda p: p["drawn"] == 10),                                                             # all-255 label
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "augment.npz"))
    args = ap.parse_args()
    from PIL import Image
    voc, _ = load_reference_loader(args.reference)
    frames = make_frames()
    F = frames["ir"].shape[0]
    out = {f"frames_{k}": v for k, v in frames.items()}
    rows = {k: [] for k in ("frame", "ratio", "nw", "nh", "flip", "bright_on", "beta", "contrast_on", "alpha", "pad_h", "pad_w", "cand",
                            "drawn", "box", "seed", "ir3", "vis3", "mask3", "label")}
    with tempfile.TemporaryDirectory() as tmp:
        for sub, key in (("Infrared", "ir"), ("Visible", "vis"), ("Mask2", "mask"), ("Label", "label")):
            os.makedirs(os.path.join(tmp, sub))
            for f in range(F):
                Image.fromarray(frames[key][f]).save(os.path.join(tmp, sub, f"f{f}.png"))
        with open(os.path.join(tmp, "train.txt"), "w") as fh:
            fh.write("".join(f"f{f}\n" for f in range(F)))
        for frame, rng_range, want in WANTED:
            ds = voc.VOC12SegDataset(root_dir=tmp, name_list_dir=tmp, split="train", stage="train", rescale_range=rng_range,
                                     crop_size=CROP, img_fliplr=True, ignore_index=255, aug=True)
            ds.color_jittor.saturation = lambda img: img
            ds.color_jittor.hue = lambda img: img
            for seed in range(100000):
                random.seed(seed)
                np.random.seed(seed)
                with Recorder() as rec:
                    name, ir3, vis3, mask3, label = ds[frame]
                p = params_from_log(rec.log, H, W)
                if want(p):
                    break
            else:
                raise RuntimeError(f"no seed gives the wanted draws for frame {frame}, range {rng_range}")
            assert name == f"f{frame}" and ir3.dtype == vis3.dtype == mask3.dtype == np.float32 and ir3.shape == (3, CROP, CROP), \
                (name, ir3.dtype, vis3.dtype, mask3.dtype, ir3.shape)
            p.update(frame=frame, seed=seed, box=p["cand"][p["drawn"] - 1], ir3=ir3, vis3=vis3, mask3=mask3, label=np.asarray(label))
            for k in rows:
                rows[k].append(p[k])
            print(f"frame {frame} seed {seed}: ratio {p['ratio']:.4f} -> {p['nh']} x {p['nw']}, flip {p['flip']}, brightness "
                  f"{p['bright_on']} {p['beta']:.3f}, contrast {p['contrast_on']} {p['alpha']:.3f}, pad ({p['pad_h']}, {p['pad_w']}), "
                  f"{p['drawn']} candidates drawn, box {p['box']}")
    for k, v in rows.items():
        out[k] = np.asarray(v)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
