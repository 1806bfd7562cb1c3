"""PNG outputs on the device: ``image_codecs.encode_png_batch`` against the restatement's bytes (tests/png_enc_ref.py) with no tolerance, on
every fixture of tests/png_enc_fixtures.py in batches that mix sizes and kinds; against itself on a second call; through this
project's own decoder; and the two commands that write PNGs, each against its ``pil`` run."""
import io

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image

import png_enc_fixtures as EF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from fusiondepth_amd import image_codecs
    return image_codecs


@pytest.fixture(scope="module")
def encoded_batches(ops):
    """[(names, arrays, files as bytes, stats)] - every fixture encoded once, from device tensors in the even batches and from host
    arrays in the odd ones."""
    out = []
    for k, part in enumerate(EF.batches()):
        names, arrays = [n for n, _ in part], [a for _, a in part]
        images = [torch.from_numpy(a).cuda() for a in arrays] if k % 2 == 0 else arrays
        files, stats = ops.encode_png_batch(images)
        assert all(isinstance(f, memoryview) for f in files)
        out.append((names, arrays, [bytes(f) for f in files], stats))
    return out


def test_batches_mix_sizes_and_kinds():
    parts = EF.batches()
    assert sorted(n for p in parts for n, _ in p) == sorted(n for n, _ in EF.images())
    for p in parts:
        assert len({n.split("-")[0] for n, _ in p}) == 3 and len({a.shape[:2] for _, a in p}) > 10


def test_files_equal_the_restatement_byte_for_byte(encoded_batches):
    want = EF.encoded()
    for names, arrays, files, stats in encoded_batches:
        for name, data in zip(names, files):
            assert data == want[name], (name, len(data), len(want[name]))
        assert stats["bytes"] == sum(len(f) for f in files)
        assert stats["raw_bytes"] == sum(a.shape[0] * (1 + a.shape[1] * a.dtype.itemsize * (3 if a.ndim == 3 else 1)) for a in arrays)


def test_two_calls_give_equal_bytes(ops, encoded_batches):
    for names, arrays, files, _ in encoded_batches:
        again, _ = ops.encode_png_batch([torch.from_numpy(a).cuda() for a in arrays])
        assert [bytes(f) for f in again] == files
        assert all(f.obj is again[0].obj for f in again) and again[0].obj.size == sum(len(f) for f in files)    # one buffer, exactly the files


def test_own_decoder_returns_the_input(ops, encoded_batches):
    for names, arrays, files, _ in encoded_batches:
        for mode, pick in (("rgb", lambda n: not n.startswith("g16")), ("gray16", lambda n: n.startswith("g16"))):
            idx = [i for i, n in enumerate(names) if pick(n)]
            frames, stats = ops.decode_png_batch([files[i] for i in idx], mode=mode)
            assert stats == {"device": len(idx), "fallback": 0}
            for f, i in zip(frames, idx):
                a = arrays[i]
                want = np.repeat(a[:, :, None], 3, 2) if names[i].startswith("g8") else a
                assert np.array_equal(f.cpu().numpy(), want), names[i]


def test_pillow_opens_the_device_s_files(encoded_batches):
    names, arrays, files, _ = encoded_batches[1]
    for name, a, data in zip(names, arrays, files):
        with Image.open(io.BytesIO(data)) as img:
            assert np.array_equal(np.asarray(img), a), name


def test_uncovered_inputs_are_refused(ops):
    ok = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((4, 4), device="cuda"), torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 4, 3), dtype=torch.uint16, device="cuda"), torch.zeros((2, 4, 4), dtype=torch.int16, device="cuda")):
        with pytest.raises(ValueError):
            ops.encode_png_batch([ok, bad])
    files, _ = ops.encode_png_batch([torch.arange(24, dtype=torch.uint8, device="cuda").view(4, 6).t()])    # a strided view
    with Image.open(io.BytesIO(bytes(files[0]))) as img:
        assert np.array_equal(np.asarray(img), np.arange(24, dtype=np.uint8).reshape(4, 6).T)


def test_payloads_that_stay_on_the_device_are_the_host_s(ops):
    """What ``--png_encoder device`` encodes: ``depth_export(want_device=True)`` (with and without ``want_depth``) and
    ``quantize_u16(want_device=True)`` - the ``--eval_gdc`` route, one map at a time - hold the values of the downloads they replace, and
    a one-image batch of each decodes to them."""
    from fusiondepth_amd import detection as D
    rng = np.random.RandomState(3)
    disps = torch.from_numpy(rng.uniform(0.02, 0.6, (3, 24, 80)).astype(np.float32)).cuda()
    sizes, ratios = [(37, 124), (36, 121), (5, 7)], rng.uniform(1.2, 1.4, 3).astype(np.float32)
    host = D.depth_export(disps, sizes, ratios=ratios)
    dev = D.depth_export(disps, sizes, ratios=ratios, want_device=True)
    dev2, depths = D.depth_export(disps, sizes, ratios=ratios, want_depth=True, want_device=True)
    for h, a, b in zip(host, dev, dev2):
        assert a.is_cuda and a.dtype == torch.uint16 and np.array_equal(a.cpu().numpy(), h) and torch.equal(a, b)
    files, _ = ops.encode_png_batch(dev)
    for h, f in zip(host, files):
        with Image.open(io.BytesIO(bytes(f))) as img:
            assert img.mode == "I;16" and np.array_equal(np.asarray(img), h)
    depth = depths[0].double() * 1.0000001                       # a float64 map, as GDC returns one; NaN, negative and too large included
    depth[0, :3] = torch.tensor([float("nan"), -1.0, 300.0], dtype=torch.float64, device="cuda")
    want = D.quantize_u16(depth)
    got = D.quantize_u16(depth, want_device=True)
    assert got.is_cuda and got.dtype == torch.uint16 and np.array_equal(got.cpu().numpy(), want) and want[0, :3].tolist() == [0, 0, 65535]
    (data,), _ = ops.encode_png_batch([got])                     # as export_detection's on_depth calls it
    with Image.open(io.BytesIO(bytes(data))) as img:
        assert np.array_equal(np.asarray(img), want)


# --------------------------------------------------------------------------------------------- the two commands
def test_export_detection_writes_the_same_maps_with_either_encoder(tmp_path_factory):
    """``--png_encoder device`` on the tiny synthetic object tree of tests/test_gpu_pseudo_lidar.py: every PNG opens in Pillow to the
    uint16 values of the ``pil`` run's PNG; the scores, the ratios and the ``--pl_name`` clouds are bit-equal."""
    import os
    import detection_tree
    from fusiondepth_amd import detection as D
    from fusiondepth_amd import export_detection as X
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    raw_root, obj_root = str(tmp_path_factory.mktemp("enc_raw")), str(tmp_path_factory.mktemp("enc_object"))
    _, obj_lines, _ = detection_tree.make_trees(raw_root, obj_root)
    lines = [obj_lines[k] for k in (3, 0, 2)]
    splits = str(tmp_path_factory.mktemp("enc_splits"))
    os.makedirs(os.path.join(splits, "detection"))
    with open(os.path.join(splits, "detection", "test.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    D.export_gt_depths_detec(obj_root, lines, "detec", os.path.join(splits, "detection", D.detec_output_name("detec")))
    torch.manual_seed(5)
    net = Trainer(MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", "2", "--height", "192",
                                            "--width", "640", "--log_dir", str(tmp_path_factory.mktemp("enc_models"))]), verbose=False)
    model = net.save_model("init")
    del net
    flags = ["--num_layers", "18", "--data_path", obj_root, "--png", "--load_weights_folder", model, "--eval_mono", "--eval_batch_size", "3",
             "--splits_dir", splits]
    pil = X.main(flags + ["--det_name", "enc_pil", "--pl_name", "pl_pil"])
    dev = X.main(flags + ["--det_name", "enc_dev", "--pl_name", "pl_dev", "--png_encoder", "device"])
    with pytest.raises(ValueError):
        X.main(flags + ["--det_name", "enc_bad", "--png_encoder", "zlib"])
    for k in range(3):
        assert np.array_equal(np.asarray(pil[k]).view(np.uint8), np.asarray(dev[k]).view(np.uint8)), k      # scores, ratios, per image
    assert len(pil[3]) == len(dev[3]) == 3
    for a, b in zip(pil[3], dev[3]):
        with Image.open(a) as ia, Image.open(b) as ib:
            pa, pb = np.asarray(ia), np.asarray(ib)
            assert ib.mode == "I;16" and pa.dtype == pb.dtype == np.uint16 and pa.shape == pb.shape
        assert np.array_equal(pa, pb) and pa.min() != pa.max(), (a, b)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() != fb.read()                        # another encoder wrote it
    for a, b in zip(pil[4], dev[4]):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), (a, b)


def test_train_log_images_writes_the_same_sheets_with_either_encoder(tmp_path_factory):
    """A short ``train --log_images`` with and without ``--png_encoder device``: each sheet decodes to the same pixels; the scalars and
    the final parameter checksum are bit-equal; a sink of the caller's keeps receiving arrays."""
    import json
    import os
    import kitti_tree
    from fusiondepth_amd import kitti_utils as KU, log_images as L, train as T
    root = str(tmp_path_factory.mktemp("enc_kitti"))
    lines = kitti_tree.make_tree(root, [("2011_09_26", "2011_09_26_drive_0001_sync", (375, 1242), (1.0, 1.0))], frames=6, down=0.35)
    splits = str(tmp_path_factory.mktemp("enc_train_splits"))
    for name, file in (("eigen_zhou", "train_files.txt"), ("eigen", "test_files.txt")):
        os.makedirs(os.path.join(splits, name))
        with open(os.path.join(splits, name, file), "w") as f:
            f.write("\n".join(lines) + "\n")
    KU.export_gt_depths(root, lines, "eigen", os.path.join(splits, "eigen", "gt_depths.npz"))
    logs = str(tmp_path_factory.mktemp("enc_logs"))
    flags = ["--num_layers", "18", "--weights_init", "scratch", "--height", "192", "--width", "640", "--batch_size", "2",
             "--data_path", root, "--png", "--log_dir", logs, "--num_workers", "4", "--num_epochs", "1", "--log_frequency", "1",
             "--splits_dir", splits, "--seed", "5", "--val_limit", "2", "--log_images"]
    pil = T.main(flags + ["--model_name", "pil"])
    assert pil.png_encoder == "pil"
    del pil
    dev = T.main(flags + ["--model_name", "device", "--png_encoder", "device"])
    assert dev.png_encoder == "device" and isinstance(dev.image_sink, L.PngSink) and dev.image_sink._thread is None
    a, b = os.path.join(logs, "pil"), os.path.join(logs, "device")
    sa, sb = [json.load(open(os.path.join(p, "train_summary.rank0.json"))) for p in (a, b)]
    assert sa["steps"] == sb["steps"] == 2 and sa["param_checksum"] == sb["param_checksum"] and sa["last_loss"] == sb["last_loss"]
    for mode in ("train", "val"):
        ra, rb = [[json.loads(l) for l in open(os.path.join(p, mode, "scalars.jsonl"))] for p in (a, b)]
        assert len(ra) == 2 and ra == rb, mode
        names = sorted(os.listdir(os.path.join(a, mode, "images")))
        assert names == sorted(os.listdir(os.path.join(b, mode, "images"))) == ["0000001_0.png", "0000002_0.png"], mode
        for name in names:
            with Image.open(os.path.join(a, mode, "images", name)) as ia, Image.open(os.path.join(b, mode, "images", name)) as ib:
                assert ib.mode == "RGB" and np.array_equal(np.asarray(ia), np.asarray(ib)), (mode, name)
            with open(os.path.join(a, mode, "images", name), "rb") as fa, open(os.path.join(b, mode, "images", name), "rb") as fb:
                assert fa.read() != fb.read()                    # another encoder wrote it
    caught = []
    dev.image_sink = lambda mode, step, sheets, tiles: caught.append((sheets, tiles))
    dev.log_pictures("train", *dev._last_io)
    (sheets, tiles), = caught
    with Image.open(L.PngSink.path(b, "train", 2, 0)) as img:
        assert isinstance(sheets, np.ndarray) and tiles and np.array_equal(sheets[0], np.asarray(img))
    with pytest.raises(ValueError):
        T.split_off_extra(["--png_encoder", "zlib"])
