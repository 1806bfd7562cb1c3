"""Writes tests/golden/conv_routes.npz: every routing answer of the convolution entry points (csrc/conv.hip) for a fixed set of
descriptors under a fixed set of fd_tuning settings - the sizes, the BatchNorm / statistics flags and the weight re-layout jobs.

tests/test_conv_routes.py requires the library to give the same answers, so that a change to how conv.hip picks a kernel family
cannot quietly change a workspace size, a weight layout or a job list.  Regenerate only when a route is meant to change:

    python tests/golden/make_conv_routes.py

The cases: every convolution of the BASELINE configurations (ResNet-18 640x192 batch 12, ResNet-50 batch 8, ResNet-18 1024x320
batch 8, the Refiner and the Completor), written down from the network definitions, plus a grid around every route threshold."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "conv_routes.npz")

DESC_FIELDS = ("N", "Cin", "H", "W", "Cout", "KH", "KW", "stride", "pad", "pad_mode", "act", "in_norm")
JOB_INT_FIELDS = ("Co", "Ci", "KH", "KW", "TA", "TB", "kh0", "dkh", "kw0", "dkw", "mode", "reserved")
MAX_JOBS = 4
# one setting per route-selecting fd_tuning field ("" = the defaults)
SETTINGS = ("", "wino_fwd=0", "wino_wgrad=0", "wino_fwd_2d_min=0", "wino_wgrad_2d=0", "wino_wgrad_2d=1",
            "reflect_ring=0", "reflect_ring=4096", "reflect_wino=0", "reflect_wino_padded_max=0",
            "conv_n16_min_pixels=-1", "conv_c1=0", "stem7=0",
            "limb_1x1=0", "limb_conv=0", "wino_wgrad_limb=0", "wino_wgrad_limb=1", "wino_fwd_limb=1",
            "wino_fwd_2d_m128=0", "wino_fwd_2d_m128=2", "wino_min_cout=64")

DEC_WIDTHS = (16, 32, 64, 128, 256)
ACT = {"none": 0, "relu": 1, "elu": 2, "sigmoid": 3, "tanh": 4}


def conv(N, Cin, H, W, Cout, K, stride=1, pad=None, refl=False, act="none", in_norm=0):
    return (N, Cin, H, W, Cout, K, K, stride, K // 2 if pad is None else pad, 1 if refl else 0, ACT[act], in_norm)


def encoder(layers, cin, N, H, W):
    """ResNet trunk (networks/resnet_encoder.py): 7x7 stem, then BasicBlock (18) or Bottleneck v1.5 (50) stages."""
    out = [conv(N, cin, H, W, 64, 7, 2, 3)]
    h, w = H // 4, W // 4
    blocks = (2, 2, 2, 2) if layers == 18 else (3, 4, 6, 3)
    exp = 1 if layers == 18 else 4
    inpl = 64
    for li, (planes, nb) in enumerate(zip((64, 128, 256, 512), blocks)):
        for bi in range(nb):
            s = (1 if li == 0 else 2) if bi == 0 else 1
            ho, wo = (h + 1) // s if s == 2 else h, (w + 1) // s if s == 2 else w
            if layers == 18:
                out += [conv(N, inpl, h, w, planes, 3, s), conv(N, planes, ho, wo, planes, 3)]
            else:
                out += [conv(N, inpl, h, w, planes, 1), conv(N, planes, h, w, planes, 3, s), conv(N, planes, ho, wo, planes * 4, 1)]
            if s != 1 or inpl != planes * exp:
                out.append(conv(N, inpl, h, w, planes * exp, 1, s, 0))
            inpl = planes * exp
            h, w = ho, wo
    return out, [64] + [p * exp for p in (64, 128, 256, 512)]


def decoder(enc, N, H, W, road=False, catxy=False, deep=False, cat2end=False, scales=(0, 1, 2, 3)):
    """DepthDecoder (networks/depth_decoder.py: decoder_layer_table): reflect-padded 3x3 blocks with ELU, sigmoid disparity heads;
    the road variant's odd input widths run zero-padded to a multiple of 16."""
    out = []
    for level in (4, 3, 2, 1, 0):
        below = enc[-1] if level == 4 else DEC_WIDTHS[level + 1]
        h, w = H >> (level + 1), W >> (level + 1)
        out.append(conv(N, below, h, w, DEC_WIDTHS[level], 3, refl=True, act="elu"))
        merged = DEC_WIDTHS[level]
        if level > 0:
            merged += enc[level - 1]
        if road and level in scales:
            merged += 6 if catxy else 3
        if road and merged % 16:
            merged = (merged + 15) // 16 * 16
        h, w = H >> level, W >> level
        if deep:
            out.append(conv(N, merged, h, w, merged, 3, refl=True, act="elu"))
            out.append(conv(N, merged, h, w, DEC_WIDTHS[level], 3, refl=True, act="elu"))
        else:
            out.append(conv(N, merged, h, w, DEC_WIDTHS[level], 3, refl=True, act="elu"))
    for s in scales:
        cin = DEC_WIDTHS[s] + (2 if (cat2end and s == 0) else 0)
        out.append(conv(N, cin, H >> s, W >> s, 1, 3, refl=True, act="sigmoid"))
    return out


def pose_decoder(enc_width, N, H, W, frames=2):
    """PoseDecoder (networks/pose_decoder.py: pose_layer_table) on the 1/32 feature map."""
    h, w = H // 32, W // 32
    return [conv(N, enc_width, h, w, 256, 1, act="relu"), conv(N, 256, h, w, 256, 3, act="relu"),
            conv(N, 256, h, w, 256, 3, act="relu"), conv(N, 256, h, w, 6 * frames, 1)]


def trainer_convs(layers, H, W, bs):
    """Depth encoder on bs frames, pose encoder on 2 x bs frame pairs (6 channels), depth and pose decoders."""
    enc, widths = encoder(layers, 3, bs, H, W)
    penc, _ = encoder(layers, 6, 2 * bs, H, W)
    return enc + penc + decoder(widths, bs, H, W) + pose_decoder(widths[-1], 2 * bs, H, W)


def network_cases():
    cases = []
    cases += trainer_convs(18, 192, 640, 12)
    cases += trainer_convs(50, 192, 640, 8)
    cases += trainer_convs(18, 320, 1024, 8)
    cases += trainer_convs(18, 352, 1216, 12)                        # Completor: full resolution 352 x 1216
    # Refiner (ResNet-18 640x192): frozen RGB / beam / pose encoders and decoders, the trained road decoder
    bs = 12
    for cin in (1, 2, 4, 5):
        cases += encoder(18, cin, bs, 192, 640)[0]
    widths = encoder(18, 3, bs, 192, 640)[1]
    cases += decoder(widths, bs, 192, 640, cat2end=True)
    for catxy in (False, True):
        for deep in (False, True):
            cases += decoder(widths, bs, 192, 640, road=True, catxy=catxy, deep=deep)
    cases += pose_decoder(widths[-1], bs, 192, 640)
    return cases


def boundary_cases():
    c = []
    for cout in (1, 2, 31, 32, 33, 63, 64, 65):                       # Cout thresholds (c1 stencil, Winograd minimum, tile heights)
        for refl in (False, True):
            c.append(conv(4, 64, 24, 80, cout, 3, refl=refl, act="sigmoid" if cout == 1 else "none"))
            c.append(conv(4, 32, 96, 320, cout, 3, refl=refl))
        c.append(conv(4, 64, 24, 80, cout, 1, pad=0))
        c.append(conv(4, 64, 24, 80, cout, 3, 2))
    for cin in range(1, 8):                                           # 7x7 stems
        for s in (1, 2):
            c.append(conv(4, cin, 64, 208, 64, 7, s, 3))
        c.append(conv(4, cin, 64, 208, 64, 7, 2, 3, in_norm=1))
    for cin in (8, 15, 16, 17, 24, 32, 48, 96):                       # Cin % 16
        c.append(conv(4, cin, 48, 160, 64, 3))
        c.append(conv(4, cin, 48, 160, 64, 3, refl=True, act="elu"))
        c.append(conv(4, cin, 48, 160, 128, 1, pad=0))
        c.append(conv(4, cin, 48, 160, 128, 3, 2))
    for cin, cout in ((128, 511), (128, 512), (128, 513), (256, 255), (256, 256), (256, 257), (255, 256), (512, 128), (1024, 64)):
        c.append(conv(8, cin, 12, 40, cout, 3))                       # Cin * Cout around 65536
        c.append(conv(8, cin, 12, 40, cout, 3, refl=True))
        c.append(conv(8, cin, 12, 40, cout, 1, pad=0))
    for h, w in ((63, 65), (64, 64), (3, 1365), (2, 2048), (45, 91), (91, 45),
                 (127, 129), (128, 128), (3, 5461), (2, 8192)):       # planes 4095 / 4096 and 16383 / 16384
        for cin, cout in ((16, 16), (32, 32), (64, 64), (128, 128)):
            c.append(conv(2, cin, h, w, cout, 3, refl=True, act="elu"))
            c.append(conv(2, cin, h, w, cout, 3))
    for w in range(76, 85):                                           # W % 4, W % 8, odd H
        for h in (24, 25):
            c.append(conv(4, 64, h, w, 64, 3))
            c.append(conv(4, 128, h, w, 128, 3, refl=True, act="elu"))
            c.append(conv(4, 256, h, w, 256, 3))
            c.append(conv(4, 256, h, w, 512, 3, 2))
            c.append(conv(4, 256, h, w, 512, 1, 2, 0))
    for k in (1, 3):                                                  # stride 2, K 1 and 3, both paddings of a 1x1
        for cin, cout in ((64, 128), (128, 256), (256, 512), (512, 1024), (256, 128), (48, 64), (64, 40)):
            for pad in ((0, 1) if k == 1 else (1, 0, 2)):
                for h, w in ((48, 160), (47, 159), (6, 20)):
                    c.append(conv(8, cin, h, w, cout, k, 2, pad))
    for act in ACT:                                                   # act
        c.append(conv(4, 64, 24, 80, 64, 3, act=act))
        c.append(conv(4, 256, 24, 80, 256, 1, pad=0, act=act))
        c.append(conv(4, 64, 24, 80, 128, 3, 2, act=act))
    for k in (1, 3, 5):                                               # in_norm, other kernels
        c.append(conv(4, 3, 64, 208, 64, k, 1, in_norm=1))
        c.append(conv(4, 16, 64, 208, 64, k, 2))
    return c


def cases():
    seen, out = set(), []
    for d in network_cases() + boundary_cases():
        if d not in seen:
            seen.add(d)
            out.append(d)
    return np.array(out, dtype=np.int32)


def evaluate(descs, settings):
    """The routing answers of the library that fusiondepth_amd._lib loads, for every (setting, case)."""
    from fusiondepth_amd import _lib, tuning
    lib = _lib.load()
    W_DUMMY, WT_DUMMY = 1 << 20, 1 << 32                              # host values only: the job calls fill structs
    ns, nc = len(settings), len(descs)
    sizes = np.zeros((ns, nc, 6), np.int64)
    bn_ok = np.zeros((ns, nc, 3), np.int8)
    njobs = np.zeros((ns, nc, 2), np.int8)
    jobs = np.zeros((ns, nc, 2, MAX_JOBS, 3 + len(JOB_INT_FIELDS) + 2), np.int64)
    arr = (_lib.RelayoutJob * MAX_JOBS)()
    for si, s in enumerate(settings):
        kw = dict((k, int(v)) for k, v in (p.split("=") for p in s.split(",") if p))
        with tuning.override(**kw):
            for ci, row in enumerate(descs):
                d = _lib.ConvDesc(*[int(v) for v in row])
                p = ctypes.byref(d)
                sizes[si, ci] = [lib.fd_conv2d_fwd_wt_floats(p), lib.fd_conv2d_fwd_ws_floats(p), lib.fd_conv2d_bwd_data_wt_floats(p),
                                 lib.fd_conv2d_bwd_data_ws_floats(p), lib.fd_conv2d_bwd_weight_ws_floats(p), lib.fd_conv2d_fwd_stat_slots(p)]
                bn_ok[si, ci] = [lib.fd_conv2d_fwd_bn_ok(p, g) for g in (1, 2, 4)]
                for kind in (0, 1):
                    ctypes.memset(arr, 0x5a, ctypes.sizeof(arr))
                    n = lib.fd_conv2d_relayout_jobs(p, kind, ctypes.c_void_p(W_DUMMY), ctypes.c_void_p(WT_DUMMY), arr)
                    assert 0 <= n <= MAX_JOBS, n
                    njobs[si, ci, kind] = n
                    for j in range(n):
                        a = arr[j]
                        jobs[si, ci, kind, j] = ([1, (a.w or 0) - W_DUMMY, (a.dst or 0) - WT_DUMMY] +
                                                 [getattr(a, f) for f in JOB_INT_FIELDS] + [a.n, a.first_block])
    return dict(sizes=sizes, bn_ok=bn_ok, njobs=njobs, jobs=jobs)


def main():
    sys.path.insert(0, ROOT)
    descs = cases()
    ans = evaluate(descs, SETTINGS)
    np.savez_compressed(OUT, desc=descs, settings=np.array(SETTINGS), **ans)
    print("%s: %d cases x %d settings, %d bytes" % (OUT, len(descs), len(SETTINGS), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
