"""Golden vectors of the depth-completion data path and scorer: runs the reference's own ``datasets.KITTICompletion``,
``get_4beam_2channel`` (gen2cha_completion.py) and ``compute_errors`` (evaluate_completion.py) on the seeded tree of
tests/completion_tree.py and the seeded pairs below, and stores what they return.

    python tests/golden/make_completion.py        # rewrites tests/golden/completion_*.npz

Runs only where the reference checkout exists (FD_REFERENCE, never on the GPU box).  Shims: ``cv2`` and ``skimage`` are stubbed
in ``sys.modules`` (imported, never called on this path); ``torchvision.transforms`` is the published torchvision -> PIL mapping of
make_augment.py (``Resize`` = ``Image.resize``, ``ColorJitter`` = ``pil_jitter`` with the injected draw, ``ToTensor`` = uint8 / 255);
``PIL.Image.ANTIALIAS = Image.LANCZOS`` (the attribute is gone in Pillow 10+); ``random.random`` returns the injected draws.
``get_4beam_2channel`` and ``compute_errors`` are lifted out of their scripts by name: gen2cha_completion.py starts a process pool
at import and evaluate_completion.py imports open3d / wandb.

Written (compressed; one file per item and mode so that each stays below the largest golden already committed):
  completion_paths.npz      the path lists of every split, relative to the tree.
  completion_<item>_<mode>.npz   item in (train, train_flip, val, test), mode in (full, pad = --completion_not_full_res): every depth key
      (``4beam``, ``depth_gt``, ``full_res_4beam``, ``2channel_<f>`` = channel 0 of ("2channel", f, 0); both channels were checked
      equal here), colour scales 2 and 3 in full (``color_<f>_<s>``, ``color_aug_<f>_<s>``) and three row strips of scales 0 and 1
      (``color_<f>_<s>_rows<r>``: 4 rows from r).  Colour planes are stored as the uint8 v of ``ToTensor``'s v / 255 (checked
      lossless here); ``color_aug`` only where the item was augmented (it equals ``color`` otherwise, checked here).
  completion_scatter.npz    ``get_4beam_2channel`` of the cropped sparse map / 100 of two items.
  completion_metrics.npz    seeded (gt, pred) pairs -> ``compute_errors`` of the selected, scaled and clamped values, np.median of both and
      their ratio (the recipe of evaluate_completion.py:297-355).
"""
import ast
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import completion_tree as CT  # noqa: E402
import make_augment as MA  # noqa: E402

REF = os.environ.get("FD_REFERENCE", "/root/reference")
JITTER = ((1.13, 0.85, 1.2, -0.07), (2, 0, 3, 1))
STRIP_ROWS = {0: (0, 173, 348), 1: (0, 87, 172)}
ITEMS = (("train", True, 1, False, False), ("train_flip", True, 4, True, True), ("val", False, 2, False, False), ("test", False, 1, False, False))
FRAMES = [0, -1, 1]
METRIC_SHAPE = (37, 53)
METRIC_COUNTS = (0, 1, 2, 301, 400)


def load_reference():
    from PIL import Image
    for name in ("cv2", "skimage", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

    class Resize:
        def __init__(self, size, interpolation):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            return img.resize((self.size[1], self.size[0]), self.interpolation)

    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(MA.pil_planes(np.asarray(img)))

    class ColorJitter:
        draw = None                                              # the injected (factors, order), one per item

        def __init__(self, *ranges):
            pass

        @staticmethod
        def get_params(*ranges):
            return None

        def __call__(self, img):
            return Image.fromarray(MA.pil_jitter(np.asarray(img), *ColorJitter.draw))

    tr.Resize, tr.ToTensor, tr.ColorJitter = Resize, ToTensor, ColorJitter
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    sys.path.insert(0, REF)
    import datasets as ref_datasets
    return ref_datasets, ColorJitter


def lifted(script, names, ns):
    src = open(os.path.join(REF, script)).read()
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    exec(compile(ast.Module(body=fns, type_ignores=[]), script, "exec"), ns)
    return [ns[n] for n in names]


def metric_pairs(seed=515):
    """N = len(METRIC_COUNTS) images of METRIC_SHAPE: image n has METRIC_COUNTS[n] pixels with gt > 0.1; the even and the odd case
    carry duplicated values across the middle of both selections."""
    rng = np.random.default_rng(seed)
    H, W = METRIC_SHAPE
    gts, preds = [], []
    for count in METRIC_COUNTS:
        gt = np.where(rng.random((H, W)) < 0.5, 0.0, rng.uniform(0.0, 0.1, (H, W))).astype(np.float32)       # below the threshold
        pred = rng.uniform(0.5, 90.0, (H, W)).astype(np.float32)
        pred[rng.random((H, W)) < 0.01] = 1e-4                                                               # below MIN_DEPTH
        at = rng.permutation(H * W)[:count]
        vals = rng.uniform(1.0, 80.0, count).astype(np.float32)
        pv = (vals * rng.uniform(0.3, 0.6, count)).astype(np.float32)
        if count > 4:
            order = np.argsort(vals)
            vals[order[count // 2 - 2:count // 2 + 2]] = vals[order[count // 2]]
            order = np.argsort(pv)
            pv[order[count // 2 - 2:count // 2 + 2]] = pv[order[count // 2]]
        gt.reshape(-1)[at] = vals
        pred.reshape(-1)[at] = pv
        gts.append(gt)
        preds.append(pred)
    return np.stack(gts), np.stack(preds)


def build():
    ref_datasets, jitter_cls = load_reference()
    get2cha, = lifted("gen2cha_completion.py", ["get_4beam_2channel"], {"torch": torch})
    compute_errors, = lifted("evaluate_completion.py", ["compute_errors"], {"np": np})
    sets = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = CT.make_tree(os.path.join(tmp, "completion"))
        rel = lambda p: "" if p is None else os.path.relpath(p, root)
        paths = {}
        for split, val_split in (("train", "select"), ("val", "select"), ("val", "full"), ("test_completion", "select")):
            got = ref_datasets.completion_dataset.get_paths_and_transform(root, split, val_split)
            for k, v in got.items():
                paths["%s_%s_%s" % (split, val_split, k)] = np.array([rel(p) for p in v])
        sets["completion_paths"] = paths
        real_random = random.random
        try:
            for mode, nfr in (("full", False), ("pad", True)):
                height, width = (192, 640) if nfr else (352, 1216)
                for name, is_train, index, do_flip, do_aug in ITEMS:
                    opt = CT.options(completion_not_full_res=nfr, completion_test=name == "test", eval_gdc=True, need_path=True)
                    ds = ref_datasets.KITTICompletion(root, height, width, FRAMES if is_train else [0], 4, is_train=is_train, val_split="select", opt=opt)
                    draws = iter([0.9 if do_aug else 0.1, 0.9 if do_flip else 0.1])
                    random.random = lambda: next(draws)
                    jitter_cls.draw = JITTER
                    it = ds[index]
                    random.random = real_random
                    out = {"path": np.array(rel(it["path"])), "date": np.array(it["date"]), "index": np.int64(index),
                           "do_flip": np.bool_(do_flip), "do_color_aug": np.bool_(do_aug)}
                    for k in ("4beam", "depth_gt", "full_res_4beam"):
                        if k in it:
                            out[k] = it[k].numpy()
                    assert np.array_equal(it["2channel"][0].numpy(), it["2channel"][1].numpy()) and np.array_equal(it["2channel"][0].numpy(), it["4beam"][0].numpy())
                    for f in (FRAMES if is_train else [0]):
                        if is_train:
                            two = it[("2channel", f, 0)].numpy()
                            assert np.array_equal(two[0], two[1])
                            out["2channel_%d" % f] = two[0]
                        for s in range(4):
                            for kind in ("color", "color_aug"):
                                a = it[(kind, f, s)].numpy()
                                if kind == "color_aug" and not do_aug:
                                    assert np.array_equal(a, it[("color", f, s)].numpy())      # stored once: the tests use ``color``
                                    continue
                                u8 = np.rint(a * 255.0).astype(np.uint8)                      # ToTensor's planes are v / 255: stored as v, lossless
                                assert np.array_equal(u8.astype(np.float32) / np.float32(255), a)
                                a = u8
                                if s >= 2:
                                    out["%s_%d_%d" % (kind, f, s)] = a
                                else:
                                    for r in STRIP_ROWS[s]:
                                        r = min(r, a.shape[1] - 4)
                                        out["%s_%d_%d_rows%d" % (kind, f, s, r)] = a[:, r:r + 4]
                    sets["completion_%s_%s" % (name, mode)] = out
        finally:
            random.random = real_random
        # the scatter of two cropped sparse maps (gen2cha_completion.py:123-126)
        sc = {}
        import completion_ref as CR
        train = ref_datasets.completion_dataset.get_paths_and_transform(root, "train", "select")
        for k, index in enumerate((1, 4)):
            png = CR.load_png(train["d"][index])
            four = torch.tensor(CR.bottom_crop(png.astype(np.float32) / 256.).copy()) / 100.0
            depth, conf = get2cha(four, height=352, width=1216)
            sc["index%d" % k], sc["depth%d" % k], sc["conf%d" % k] = np.int64(index), depth.numpy(), conf.numpy()
        sets["completion_scatter"] = sc
    gt, pred = metric_pairs()
    me = {"seed": np.int64(515)}
    for n in range(len(gt)):
        mask = gt[n] > 0.1
        if not mask.any():
            continue
        for tag, scale in (("", 1.0), ("_s", 1.3)):
            p = pred[n].copy()
            p *= scale
            ratio = np.median(gt[n][mask]) / np.median(p[mask])
            me["median_gt%d%s" % (n, tag)], me["median_pred%d%s" % (n, tag)], me["ratio%d%s" % (n, tag)] = np.median(gt[n][mask]), np.median(p[mask]), ratio
            p *= ratio
            ps, g = p[mask], gt[n][mask]
            ps[ps < 1e-3] = 1e-3
            ps[ps > 80] = 80
            me["errors%d%s" % (n, tag)] = np.array(compute_errors(g, ps), dtype=np.float64)
    sets["completion_metrics"] = me
    return sets


if __name__ == "__main__":
    limit = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and not f.startswith("completion_"))
    for stem, arrays in build().items():
        colour = {k: v for k, v in arrays.items() if k.startswith("color")}         # an item's colour keys go to <stem>.part1.npz, as
        parts = [(stem, {k: v for k, v in arrays.items() if k not in colour})]      # losses_b2_64x96.part*.npz are split (conftest.golden)
        if colour:
            parts.append((stem + ".part1", colour))
        for name, part in parts:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **part)
            size = os.path.getsize(path)
            print("%s: %d bytes" % (path, size))
            assert size < limit, "%s is larger than the largest golden already committed (%d bytes): split it" % (path, limit)
