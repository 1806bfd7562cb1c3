"""Golden vectors of the LiDAR sparsifier: runs the reference's own ``gen_sparse_points`` / ``pto_ang_map`` (sparsify/sparsify.py)
on the seeded scans of tests/sparsify_ref.py and stores what they return as integers.

Runs only where the reference checkout exists (FD_REFERENCE, never on the GPU box), under numpy 2.  ``cv2`` - imported by the
reference's ``data_utils`` for functions the sparsifier never calls - is stubbed in ``sys.modules``.

Written:
  sparsify_clean.npz / sparsify_full.npz   one scan each.  "clean" has the near-edge points (sparsify_ref.near_edge at W = 1024,
      which contains those at W = 512) removed, "full" keeps them.  Keys: ``removed`` (indices deleted from the seed's scan),
      ``n_points``, ``kept`` (indices that pass the reference's filter), ``row`` / ``col_w1024`` / ``col_w512`` (the reference's cell
      per kept point), ``near`` (near-edge kept points, positions into ``kept``), ``out_<config>`` (index into the scan of every
      output point, in the reference's order).
  sparsify_edge.npz    the hand-made scans (a few points each): ``<scan>__<config>`` the float32 output points themselves, as the
      reference writes them to disk; ``<scan>__row`` / ``<scan>__col`` cells at W = 1024.
  sparsify_line_specs.json   settings only: the --line_spec / --W / --H / --nbeams / --random_sample of the prepare scripts.

The output points are identified by their intensity: the scan handed to the reference carries the point index there (exact in
float32 below 2^24).  Cells and winners do not read the intensity; the random-sample norm does, but no point of the synthetic scans
has x = y = z = 0.  The hand-made scans, where an all-zero point matters, go through the reference as they are.
"""
import json
import os
import re
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sparsify_ref as SR  # noqa: E402

REF = os.environ.get("FD_REFERENCE", "/root/reference")


def load_reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, os.path.join(REF, "sparsify"))
    import sparsify as ref_sparsify
    return ref_sparsify


def run_reference(ref, scan, cfg, tmp, coded=True):
    """gen_sparse_points on ``scan`` written as a KITTI file -> the indices of its output points (``coded``: through the intensity
    channel), or the float32 output points themselves."""
    coded, as_is = scan.copy(), not coded
    if not as_is:
        coded[:, 3] = np.arange(len(scan), dtype=np.float32)
    folder = "2011_09_26/2011_09_26_drive_0001_sync"
    d = os.path.join(tmp, folder, "velodyne_points", "data")
    os.makedirs(d, exist_ok=True)
    coded.tofile(os.path.join(d, "%010d.bin" % 7))
    args = types.SimpleNamespace(ptc_path=tmp + "/", H=64, W=cfg["W"], slice=cfg.get("slice", 1), line_spec=cfg.get("line_spec"),
                                 random_sample=cfg.get("random_sample", 0), fill_in_map_dir=None, fill_in_spec=None, fill_in_slice=None,
                                 store_line_map_dir=None)
    if "np_seed" in cfg:
        np.random.seed(cfg["np_seed"])
    out = ref.gen_sparse_points(folder + " 7 l", args)
    if as_is:
        return out.astype(np.float32).reshape(-1, 4)          # sparse_and_save's cast
    idx = out[:, 3].astype(np.int64)
    assert np.array_equal(out[:, :3].astype(np.float32), scan[idx, :3])
    return idx


def cells_through_reference(ref, p, W):
    """Cell of every point of the filtered scan ``p`` as the reference computes it.  ``pto_ang_map`` does not return its cell
    indices, so its first lines (sparsify.py:41-58) are executed from the reference's own source text on ``p``."""
    import inspect
    src = inspect.getsource(ref.pto_ang_map).split("\n")
    start = next(i for i, l in enumerate(src) if "dtheta = " in l)
    stop = next(i for i, l in enumerate(src) if "depth_map = - np.ones" in l)
    body = "\n".join(l[4:] for l in src[start:stop])
    ns = {"np": np, "velo_points": p, "H": 64, "W": W}
    exec(body, ns)
    return ns["theta_"].astype(np.int64), ns["phi_"].astype(np.int64)


def scan_fixture(ref, kind, tmp):
    scan = SR.synthetic_scan(SR.FIXTURE_SEEDS[kind])
    removed = np.zeros(0, dtype=np.int64)
    if kind == "clean":
        kept = np.flatnonzero(SR.filter_mask(scan))
        removed = kept[SR.near_edge(scan[kept], 64, 1024)]
        scan = np.delete(scan, removed, axis=0)
    kept = np.flatnonzero(SR.filter_mask(scan))
    p = scan[kept]
    out = {"removed": removed.astype(np.int32), "n_points": np.int64(len(scan)), "kept": kept.astype(np.int32)}
    for W in (1024, 512):
        row, col = cells_through_reference(ref, p, W)
        out["row"] = row.astype(np.uint8)
        out["col_w%d" % W] = col.astype(np.uint16)
    out["near"] = np.flatnonzero(SR.near_edge(p, 64, 1024)).astype(np.int32)
    for name, cfg in SR.CONFIGS.items():
        out["out_" + name] = run_reference(ref, scan, cfg, tmp).astype(np.int32)
    print("%s: %d points, %d kept, %d near an edge (%.2e), %d removed" % (kind, len(scan), len(kept), len(out["near"]),
                                                                          len(out["near"]) / len(kept), len(removed)))
    return out


def edge_fixture(ref, tmp):
    out = {}
    for sname, scan in SR.edge_scans().items():
        kept = np.flatnonzero(SR.filter_mask(scan))
        row, col = cells_through_reference(ref, scan[kept], 1024) if len(kept) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        out[sname + "__row"], out[sname + "__col"] = row.astype(np.int32), col.astype(np.int32)
        for cname, cfg in SR.EDGE_CONFIGS.items():
            out["%s__%s" % (sname, cname)] = run_reference(ref, scan, cfg, tmp, coded=False)
    return out


def line_specs():
    """The settings of the prepare scripts' sparsify.py lines."""
    out = {}
    for name in sorted(os.listdir(REF)):
        if not (name.startswith("prepare_") and name.endswith(".sh")):
            continue
        lines = [l for l in open(os.path.join(REF, name)).read().split("\n") if "sparsify.py" in l]
        if not lines:
            continue
        settings = set()
        for l in lines:
            flags = re.sub(r"--split_file \S+", "", l.split("sparsify.py", 1)[1]).split()
            settings.add(" ".join(flags))
        assert len(settings) == 1, (name, settings)
        toks = settings.pop().split()
        entry, key = {}, None
        for t in toks:
            if t.startswith("--"):
                key = t[2:]
                entry[key] = []
            else:
                entry[key].append(int(t))
        out[name] = {k: (v if k == "line_spec" else v[0]) for k, v in entry.items()}
    return out


def main():
    assert int(np.__version__.split(".")[0]) >= 2, "the fixtures pin numpy 2 semantics"
    ref = load_reference()
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("clean", "full"):
            np.savez_compressed(os.path.join(HERE, "sparsify_%s.npz" % kind), **scan_fixture(ref, kind, tmp))
        np.savez_compressed(os.path.join(HERE, "sparsify_edge.npz"), **edge_fixture(ref, tmp))
    with open(os.path.join(HERE, "sparsify_line_specs.json"), "w") as f:
        json.dump(line_specs(), f, indent=1, sort_keys=True)
        f.write("\n")
    for n in ("sparsify_clean.npz", "sparsify_full.npz", "sparsify_edge.npz", "sparsify_line_specs.json"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
