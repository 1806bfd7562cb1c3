"""Convert a KITTI PNG tree to JPEG, the step the reference's README does with ImageMagick before anything else
(``convert -quality 92 -sampling-factor 2x2,1x1,1x1 x.png x.jpg && rm x.png``):

    python -m fusiondepth_amd.convert_frames --data_path D [--out_path O] [--quality 92] [--sampling 2x2] [--encoder device|pil]
                                             [--png_decoder device|pil] [--delete_png] [--overwrite] [--batch 36] [--workers 16]

    Every ``*.png`` under ``D``, in sorted order, becomes ``<same path>.jpg`` (under ``O`` if given), written through a temporary name
    and a rename on the host pool.  A batch is decoded with ``image_codecs.decode_png_batch(mode="rgb")`` and encoded with
    ``image_codecs.encode_jpeg_batch``: the frames stay on the device between the two codecs.  ``--delete_png`` removes a PNG only after
    its JPEG has been renamed into place.  An existing ``.jpg`` is skipped without ``--overwrite``; a 16-bit PNG (depth ground truth
    under the same root) is skipped, never converted and never deleted, and reported; an 8-bit grey PNG becomes a greyscale JPEG
    through Pillow.  ``--encoder pil --png_decoder pil`` gives the same files from Pillow alone.

    DEVIATION: the files equal Pillow's ``save(quality=q, subsampling=s)``, not ImageMagick's - ImageMagick writes other header
    segments; the coefficients come from the same libjpeg rules, which is not claimed bit for bit.

Prints one summary line and returns a dict with the same fields: converted, device, fallback, skipped, deleted, bytes_in, bytes_out."""
import argparse
import concurrent.futures
import json
import os
import threading

from . import image_codecs

SKIP_MODES = ("I;16", "I;16B", "I;16L", "I;16N", "I", "F")       # Pillow's modes of a 16-bit (or wider) single-channel PNG


def find_pngs(root):
    out = []
    for d, dirs, names in os.walk(root):
        dirs.sort()
        out += [os.path.join(d, n) for n in names if n.endswith(".png")]
    return sorted(out)


def classify(path):
    """-> 'skip' (16-bit), 'grey' (8-bit grey: Pillow writes a greyscale JPEG) or 'rgb'."""
    from PIL import Image
    with Image.open(path) as img:                                # the header alone
        mode = img.mode
    return "skip" if mode in SKIP_MODES else ("grey" if mode == "L" else "rgb")


def _write(dst, data, png, delete):
    """``data`` at ``dst`` through a temporary name and a rename; then, and only then, the PNG goes.  -> 1 if it was deleted."""
    os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
    tmp = "%s.tmp%d_%d" % (dst, os.getpid(), threading.get_ident())
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, dst)
    if delete:
        os.remove(png)
        return 1
    return 0


def _pil_file(path, kind, quality, sampling):
    import numpy as np
    from PIL import Image
    with Image.open(path) as img:
        a = np.asarray(img if kind == "grey" else img.convert("RGB"))
    return image_codecs.pil_jpeg(a, quality, sampling)


def convert(data_path, out_path=None, quality=92, sampling="2x2", encoder="device", png_decoder="device", delete_png=False, overwrite=False,
            batch=36, workers=16):
    for name, v in (("--encoder", encoder), ("--png_decoder", png_decoder)):
        if v not in image_codecs.JPEG_ENCODERS:
            raise ValueError("convert_frames: %s must be 'pil' or 'device', got %r" % (name, v))
    image_codecs.check_jpeg_params(quality, sampling, 1, "convert_frames")
    if not isinstance(sampling, str):
        raise ValueError("convert_frames: --sampling is one name for the whole tree")
    if batch < 1 or workers < 1:
        raise ValueError("convert_frames: --batch and --workers must be positive")
    if not os.path.isdir(data_path):
        raise ValueError("convert_frames: %s is not a directory" % data_path)
    res = {"converted": 0, "device": 0, "fallback": 0, "skipped": 0, "deleted": 0, "bytes_in": 0, "bytes_out": 0, "skipped_16bit": []}
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        todo = []
        pngs = find_pngs(data_path)
        targets = [os.path.join(out_path, os.path.relpath(p, data_path))[:-4] + ".jpg" if out_path else p[:-4] + ".jpg" for p in pngs]
        kinds = list(pool.map(lambda pt: "done" if (not overwrite and os.path.exists(pt[1])) else classify(pt[0]), zip(pngs, targets)))
        for p, t, k in zip(pngs, targets, kinds):
            if k in ("done", "skip"):
                res["skipped"] += 1
                if k == "skip":
                    res["skipped_16bit"].append(os.path.relpath(p, data_path))
            else:
                todo.append((p, t, k))
        writes = []
        for at in range(0, len(todo), batch):
            part = todo[at:at + batch]
            res["bytes_in"] += sum(os.path.getsize(p) for p, _, _ in part)
            rgb = [i for i, (_, _, k) in enumerate(part) if k == "rgb"]
            files = [None] * len(part)
            if encoder == "device" and rgb:
                if png_decoder == "device":
                    frames, _ = image_codecs.decode_png_batch([part[i][0] for i in rgb], pool=pool, mode="rgb")
                else:
                    import numpy as np
                    from PIL import Image

                    def load(path):
                        with Image.open(path) as img:
                            return np.asarray(img.convert("RGB"))
                    frames = list(pool.map(load, [part[i][0] for i in rgb]))
                enc, stats = image_codecs.encode_jpeg_batch(frames, quality=quality, sampling=sampling, pool=pool)
                for i, f in zip(rgb, enc):
                    files[i] = f
                res["device"] += stats["device"]
                res["fallback"] += stats["fallback"]
            rest = [i for i in range(len(part)) if files[i] is None]      # grey frames, and every frame of --encoder pil
            for i, data in zip(rest, pool.map(lambda i: _pil_file(part[i][0], part[i][2], quality, sampling), rest)):
                files[i] = data
            res["fallback"] += len(rest)
            for w in writes:                                     # at most one batch of writes in flight (their futures keep its buffer alive)
                res["deleted"] += w.result()
            writes = [pool.submit(_write, t, f, p, delete_png) for (p, t, _), f in zip(part, files)]
            res["converted"] += len(part)
            res["bytes_out"] += sum(len(f) for f in files)
        for w in writes:
            res["deleted"] += w.result()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m fusiondepth_amd.convert_frames", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_path", required=True)
    ap.add_argument("--out_path", default=None)
    ap.add_argument("--quality", type=int, default=92)
    ap.add_argument("--sampling", default="2x2")
    ap.add_argument("--encoder", default="device")
    ap.add_argument("--png_decoder", default="device")
    ap.add_argument("--delete_png", action="store_true")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--batch", type=int, default=36)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args(argv)
    res = convert(a.data_path, a.out_path, a.quality, a.sampling, a.encoder, a.png_decoder, a.delete_png, a.overwrite, a.batch, a.workers)
    print("convert_frames: " + json.dumps({k: v for k, v in res.items() if k != "skipped_16bit"}) +
          ("  16-bit PNGs left alone: %s" % ", ".join(res["skipped_16bit"][:8]) + (" ..." if len(res["skipped_16bit"]) > 8 else "")
           if res["skipped_16bit"] else ""))
    return res


if __name__ == "__main__":
    main()
