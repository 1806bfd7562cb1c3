"""numpy restatement of the reference's image summaries (trainer.py:656-681) for the tests of ``fd_log_sheets``: the layout of the
contact sheet, the quantisation, ``utils.normalize_image``, the automask and the assembly of a sheet from given float tiles.  A helper,
not a test.  The warp behind the colour predictions is NOT restated: those tiles are handed in (tests/test_gpu_log_images.py holds them
to the project's materialised warp instead).

Every element-wise step is one float32 numpy operation.  tests/test_log_images_cpu.py holds ``normalize_image`` against the reference's
torch expression bit for bit; the quantisation is the rule ``torch.utils.tensorboard.summary.image`` applies to float input, stated in
fusiondepth_amd/log_images.py's docstring (tensorboard is not available here to hold it against)."""
import numpy as np

F32 = np.float32


def quantise(x):
    """``trunc(min(max(x * 255, 0), 255))`` in float32, NaN -> 0 -> uint8."""
    with np.errstate(all="ignore"):
        s = np.asarray(x, F32) * F32(255.0)
        s = np.where(np.isnan(s), F32(0.0), np.minimum(np.maximum(s, F32(0.0)), F32(255.0)))
    return np.trunc(s).astype(np.uint8)


def normalize_image(x):
    """utils.normalize_image for a float32 array -> (float32 array, mi, ma): ``ma``, ``mi`` as float32, their difference in float64
    (``float(x.max()) - float(x.min())`` of Python floats), ``1e5`` where they are equal, rounded to float32 once (torch turns the
    Python scalar into the tensor's dtype), then ``(x - mi) / d`` in float32."""
    x = np.asarray(x, F32)
    ma, mi = x.max(), x.min()                                     # a NaN anywhere makes both NaN, as torch's max() / min()
    d = np.float64(ma) - np.float64(mi) if ma != mi else np.float64(1e5)
    with np.errstate(all="ignore"):
        return ((x - F32(mi)) / F32(d)).astype(F32), F32(mi), F32(ma)


def automask(sel, n_id):
    """``Outputs.__missing__``'s ``(sel > n_id - 1).float()`` through the quantisation: 255 or 0."""
    return np.where(np.asarray(sel).astype(np.int64) > int(n_id) - 1, 255, 0).astype(np.uint8)


def layout(frame_ids, scales, height, width, automask=True, predictive_mask=False, val=False, mask_size=None):
    """One item's tiles -> (Hs, Ws, [(tag without the item index, y, x, h, w, channels)]).  A row block per scale, as tall as its
    tallest tile; the tiles side by side from x = 0.  ``mask_size``: the (h, w) of the automask planes, None: scale 0's,
    "scale": the scale's own."""
    tiles, y, Ws = [], 0, 0
    for s in scales:
        h, w = height // 2 ** s, width // 2 ** s
        row = [("color_%s_%d" % (f, s), h, w, 3) for f in frame_ids]
        if s == 0:
            row += [("color_pred_%s_%d" % (f, s), h, w, 3) for f in frame_ids if f != 0]
        row += [("disp_%d" % s, h, w, 1)]
        if predictive_mask and not val:
            row += [("predictive_mask_%s_%d" % (f, s), h, w, 1) for f in frame_ids[1:]]
        if automask and not predictive_mask and not val:
            row += [("automask_%d" % s,) + ((h, w) if mask_size == "scale" else ((height, width) if mask_size is None else tuple(mask_size))) + (1,)]
        x = 0
        for tag, th, tw, ch in row:
            tiles.append((tag, y, x, th, tw, ch))
            x += tw
        Ws = max(Ws, x)
        y += max(t[1] for t in row)
    return y, Ws, tiles


def assemble(tiles, planes):
    """One sheet from ``layout``'s tiles and ``{tag: array}``: a [3,h,w] float array is quantised per channel, a [h,w] float array is
    quantised and replicated, a uint8 array ([h,w] or [h,w,3]) is taken as it is.  Bytes outside every tile are 0."""
    Hs = max(y + h for _, y, x, h, w, _ in tiles)                 # the blocks are as tall as their tallest tile
    Ws = max(x + w for _, y, x, h, w, _ in tiles)
    sheet = np.zeros((Hs, Ws, 3), np.uint8)
    for tag, y, x, h, w, ch in tiles:
        p = np.asarray(planes[tag])
        if p.dtype != np.uint8:
            p = quantise(p)
            if p.ndim == 3:
                p = p.transpose(1, 2, 0)
        if p.ndim == 2:
            p = np.repeat(p[:, :, None], 3, axis=2)
        assert p.shape == (h, w, 3), (tag, p.shape, (h, w))
        sheet[y:y + h, x:x + w] = p
    return sheet


def restate(inputs, outputs, frame_ids, scales, j, preds=None, automask_on=True, predictive_mask=False, val=False, mask_size=None):
    """The sheet of item ``j`` from numpy copies of the dicts -> (sheet, {disparity tag: (mi, ma)}).  ``preds``: {f: [3,h,w] float or
    [h,w,3] uint8} for the colour predictions (not restated here)."""
    h0, w0 = inputs[("color", frame_ids[0], scales[0])].shape[2:]
    height, width = h0 * 2 ** scales[0], w0 * 2 ** scales[0]
    Hs, Ws, tiles = layout(frame_ids, scales, height, width, automask_on, predictive_mask, val, mask_size)
    planes, stats = {}, {}
    for s in scales:
        for f in frame_ids:
            planes["color_%s_%d" % (f, s)] = inputs[("color", f, s)][j]
            if s == 0 and f != 0:
                planes["color_pred_%s_%d" % (f, s)] = preds[f]
        norm, mi, ma = normalize_image(outputs[("disp", s)][j, 0])
        planes["disp_%d" % s], stats["disp_%d" % s] = norm, (mi, ma)
        if predictive_mask and not val:
            for i, f in enumerate(frame_ids[1:]):
                planes["predictive_mask_%s_%d" % (f, s)] = outputs["predictive_mask"][("disp", s)][j, i]
        if automask_on and not predictive_mask and not val:
            sel, n_id = outputs[("sel", s)]
            planes["automask_%d" % s] = automask(sel[j], n_id)
    sheet = assemble(tiles, planes)
    assert sheet.shape == (Hs, Ws, 3)
    return sheet, stats
