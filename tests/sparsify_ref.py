"""The reference's LiDAR sparsifier (sparsify/sparsify.py:32-136, gen_sparse_points + pto_ang_map) restated in numpy in this
project's own words, the seeded synthetic scans the sparsify fixtures are made of, and the near-edge rule.

Semantics pinned: numpy 2.  ``np.radians(45.)`` is a float64 scalar and NEP 50 promotes ``radians(45.) - arcsin(y / r)`` to float64,
so distances and the two arcsines are float32 and everything after them float64 (numpy 1.x would have stayed in float32).

``tests/golden/make_sparsify.py`` runs the reference itself on these scans and stores what it returns as integers (cell per
point, index of every output point); the scans are regenerated here from their seeds.
"""
import numpy as np

BOX = (0.0, 120.0, -50.0, 50.0, -2.5, 1.5)
EDGE_SPACINGS = 8            # near-edge rule: numpy's float32 arcsin is up to 3 spacings off the correctly rounded value, the device at
#                              most half a spacing, and a factor of 2 on top
NEAR_EDGE_CAP = 0.002        # share of the filtered scan that may be near an edge

# name -> arguments of the reference (H = 64 throughout); "np_seed" seeds np.random for the random-sample draws
CONFIGS = {
    "beam1": dict(W=1024, line_spec=[9]),
    "beam2": dict(W=1024, line_spec=[9, 11]),
    "beam3": dict(W=1024, line_spec=[7, 9, 11]),
    "beam4": dict(W=1024, line_spec=[2, 7, 12, 16]),
    "slice2": dict(W=1024, slice=2),
    "beam4_w512": dict(W=512, line_spec=[2, 7, 12, 16]),
    "slice2_w512": dict(W=512, slice=2),
    "random100": dict(W=1024, random_sample=100, np_seed=100),
    "random200": dict(W=1024, random_sample=200, np_seed=200),
}
# the hand-made scans: four beams, every row, and random sampling with N = 1 (N * 1.8 / n_keep stays below 1 on a handful of points)
EDGE_CONFIGS = {"beam4": CONFIGS["beam4"], "all": dict(W=1024), "random1": dict(W=1024, random_sample=1, np_seed=5)}
FIXTURE_SEEDS = {"clean": 2011, "full": 2012}


# ---- scans ----------------------------------------------------------------------------------------------------------------------
def synthetic_scan(seed, rings=64, steps=2048):
    """A 64-ring scan of a street: ground plane 1.73 m below the sensor, walls and boxes in azimuth sectors, a far backdrop.
    About rings * steps points all round the car (half of them ahead of it), float32 [n,4]."""
    rng = np.random.default_rng(seed)
    elev = np.radians(2.0 - 0.4 * (np.arange(rings) + 0.5) + rng.uniform(-0.12, 0.12, rings))       # one bin per ring, jittered
    az = np.linspace(-np.pi, np.pi, steps, endpoint=False)
    E = elev[:, None] + rng.normal(0.0, np.radians(0.01), (rings, steps))
    A = az[None, :] + rng.normal(0.0, np.radians(0.01), (rings, steps))
    horiz = np.full((rings, steps), np.inf)                                # horizontal range of the first hit
    ground = np.where(np.tan(E) < 0, -1.73 / np.minimum(np.tan(E), -1e-9), np.inf)
    horiz = np.minimum(horiz, ground)
    for _ in range(40):                                                    # obstacles: an azimuth sector at one distance, up to a height
        a0 = rng.uniform(-np.pi, np.pi)
        width = rng.uniform(0.02, 0.5)
        dist = rng.uniform(3.0, 60.0)
        top = rng.uniform(-1.0, 1.4)
        inside = np.abs(np.angle(np.exp(1j * (A - a0)))) < width / 2
        zhit = dist * np.tan(E)
        hit = inside & (zhit > -1.73) & (zhit < top) & (dist < horiz)
        horiz = np.where(hit, dist, horiz)
    backdrop = 75.0 + 10.0 * np.sin(3 * A)
    zhit = backdrop * np.tan(E)
    horiz = np.where((backdrop < horiz) & (zhit < 1.45), backdrop, horiz)
    ok = np.isfinite(horiz) & (horiz < 115.0)
    horiz = horiz * (1.0 + rng.normal(0.0, 0.002, horiz.shape))
    x, y, z = horiz * np.cos(A), horiz * np.sin(A), horiz * np.tan(E)
    pts = np.stack([x, y, z, rng.random((rings, steps))], -1)
    # a spinning sensor delivers azimuth-major order: all rings of one step, then the next
    pts = pts.transpose(1, 0, 2)[ok.T]
    return np.ascontiguousarray(pts.astype(np.float32))


def edge_scans():
    """Hand-made cases, name -> float32 [n,4]."""
    f = lambda rows: np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    return {
        "empty": f([]),
        "outside": f([[-1.0, 0.0, 0.0, 0.5], [130.0, 0.0, 0.0, 0.5], [10.0, 60.0, 0.0, 0.5], [10.0, 0.0, 2.0, 0.5], [10.0, 0.0, -3.0, 0.5]]),
        "one": f([[12.5, -3.25, -1.5, 0.25]]),
        # the all-zero point passes the filter: d = r = 0 become 1e-6; its float64 norm is 0, so random sampling never keeps it
        "zero": f([[0.0, 0.0, 0.0, 0.0], [20.0, 1.0, -1.0, 0.3], [0.0, 0.0, 0.0, 0.7], [0.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]),
        "duplicates": f([[15.0, 2.0, -1.2, 0.1]] * 5 + [[15.0, 2.0, -1.2, 0.9]] + [[30.0, -4.0, -1.0, 0.2]] * 3),
        "bounds": f([[0.0, 5.0, -1.0, 0.1], [120.0, 5.0, -1.0, 0.1], [np.nextafter(np.float32(120.0), np.float32(0.0)), 5.0, -1.0, 0.2],
                     [10.0, -50.0, -1.0, 0.3], [10.0, 50.0, -1.0, 0.3], [60.0, np.nextafter(np.float32(50.0), np.float32(0.0)), -1.0, 0.4],
                     [10.0, 1.0, -2.5, 0.5], [10.0, 1.0, 1.5, 0.5], [40.0, 1.0, np.nextafter(np.float32(1.5), np.float32(0.0)), 0.6]]),
        # angles beyond the grid: above +2 degrees / below -23.6 degrees elevation, beyond +-45 degrees azimuth
        "clamped": f([[1.0, 0.0, 1.4, 0.1], [1.0, 0.1, -2.0, 0.2], [0.1, 10.0, -0.05, 0.3], [0.1, -10.0, -0.05, 0.4], [0.0, 3.0, -0.5, 0.5],
                      [0.0, -3.0, -0.5, 0.6], [2.0, 2.5, 1.0, 0.7], [2.0, -2.5, -2.4, 0.8]]),
    }


# ---- the sparsifier ---------------------------------------------------------------------------------------------------------------
def filter_mask(scan, box=BOX):
    x, y, z = scan[:, 0], scan[:, 1], scan[:, 2]
    return (x >= box[0]) & (x < box[1]) & (y >= box[2]) & (y < box[3]) & (z >= box[4]) & (z < box[5])


def quotients(p):
    """float32 y / r and z / d, with the zero distances replaced."""
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rr = x * x + y * y
    dd = rr + z * z
    r, d = np.sqrt(rr), np.sqrt(dd)
    r = np.where(r == 0, np.float32(0.000001), r)
    d = np.where(d == 0, np.float32(0.000001), d)
    return y / r, z / d


def bin_coordinates(qy, qz, H, W, asin32=True):
    """float64 (column, row) coordinates before truncation.  ``asin32``: arcsin in float32 (what numpy computes for the reference);
    otherwise in float64 on the same float32 quotient (the recomputation the near-edge rule is stated on)."""
    if asin32:
        ay, az = np.arcsin(qy).astype(np.float64), np.arcsin(qz).astype(np.float64)
    else:
        ay, az = np.arcsin(qy.astype(np.float64)), np.arcsin(qz.astype(np.float64))
    return (np.radians(45.0) - ay) / np.radians(90.0 / W), (np.radians(2.0) - az) / np.radians(0.4 * 64.0 / H)


def cells(p, H=64, W=1024):
    """(row, column) of every point of an already filtered scan."""
    qy, qz = quotients(p)
    c, r = bin_coordinates(qy, qz, H, W)
    return np.clip(np.trunc(r), 0, H - 1).astype(np.int64), np.clip(np.trunc(c), 0, W - 1).astype(np.int64)


def near_edge_dims(p, H=64, W=1024):
    """Per point of a filtered scan and per dimension: is the float64-recomputed bin coordinate within EDGE_SPACINGS float32 spacings
    of the arcsin value, divided by the bin width, of an integer k - and that k.  Returns ((near_col, k_col), (near_row, k_row)).
    Edges the clamp removes (0 and below, the grid's size and above) do not count."""
    qy, qz = quotients(p)
    c, r = bin_coordinates(qy, qz, H, W, asin32=False)
    out = []
    for coord, q, n, step in ((c, qy, W, np.radians(90.0 / W)), (r, qz, H, np.radians(0.4 * 64.0 / H))):
        spacing = np.spacing(np.abs(np.arcsin(q.astype(np.float64))).astype(np.float32)).astype(np.float64)
        k = np.rint(coord)
        out.append(((np.abs(coord - k) <= EDGE_SPACINGS * spacing / step) & (k >= 1) & (k <= n - 1), k.astype(np.int64)))
    return tuple(out)


def near_edge(p, H=64, W=1024):
    """Boolean per point: near an edge in either dimension."""
    (near_col, _), (near_row, _) = near_edge_dims(p, H, W)
    return near_col | near_row


def selected_rows(H=64, line_spec=None, slice=1):
    return [int(r) for r in line_spec] if line_spec is not None else list(range(0, H, slice))


def winners(row, col, rows, W, n_rows_total=64):
    """Indices (into the filtered scan) of the output points: per occupied cell of the selected rows the LAST point that fell into
    it, cells in the order rows-as-listed then columns."""
    last = np.full(n_rows_total * W, -1, dtype=np.int64)
    flat = row * W + col
    np.maximum.at(last, flat, np.arange(len(flat)))
    grid = last.reshape(n_rows_total, W)[np.asarray(rows, dtype=np.int64)].reshape(-1)
    return grid[grid >= 0]


def random_keep(points, N, uniforms):
    """Mask over the compacted points: a non-zero float64 norm and u < N * 1.8 / n_keep."""
    p = np.asarray(points, dtype=np.float64)
    nonzero = (p * p).sum(1) > 0
    n_keep = int(nonzero.sum())
    if n_keep == 0:
        return nonzero
    return nonzero & (np.asarray(uniforms, dtype=np.float64)[:len(p)] < float(N * 1.8) / n_keep)


def sparsify_indices(scan, H=64, W=1024, line_spec=None, slice=1, random_sample=0, uniforms=None, np_seed=None, cell_override=None):
    """Indices into ``scan`` of the reference's output points, in its order.  ``cell_override`` = (row, col) per filtered point replaces
    the cell computation (the device's own cells)."""
    keep = np.flatnonzero(filter_mask(scan))
    p = scan[keep]
    row, col = cells(p, H, W) if cell_override is None else cell_override
    rows = selected_rows(H, line_spec, slice)
    idx = keep[winners(np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64), rows, W, H)]
    if random_sample:
        if uniforms is None:
            np.random.seed(np_seed)
            uniforms = np.random.uniform(0, 1, len(idx))
        idx = idx[random_keep(scan[idx], random_sample, uniforms)]
    return idx


def config_uniforms(cfg, m):
    """The draws the reference makes for a random-sample configuration on m compacted points."""
    np.random.seed(cfg["np_seed"])
    return np.random.uniform(0, 1, m)


def fixture_scan(kind, removed=None):
    """The scan of the "clean" / "full" fixture: its seed's scan, minus the stored indices."""
    scan = synthetic_scan(FIXTURE_SEEDS[kind])
    if removed is not None and len(removed):
        scan = np.delete(scan, np.asarray(removed, dtype=np.int64), axis=0)
    return scan
