/* libfdhip — C ABI of the MI355X-native (gfx950) FusionDepth training hot path.
 *
 * The reference (AutoAILab/FusionDepth) has no FFI layer: its boundary is the Python module API in
 * layers.py / networks/*.py / trainer.py, whose arithmetic is implicit ATen/cuDNN calls.  Each entry
 * point below replaces one such call site (cited as reference file:line).  `fusiondepth_amd` binds
 * these with ctypes (fusiondepth_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every tensor is float32, contiguous, NCHW unless stated; pointers are DEVICE pointers owned by
 *     the caller (PyTorch caching allocator); the library never allocates device memory and keeps
 *     no state besides the last-error string.  Workspaces are passed in with their size in floats.
 *   - `stream` is a hipStream_t; every call is asynchronous and stream-ordered, no implicit sync.
 *   - return 0 on success; a hipError_t (>0) for launch failures; -1 for bad arguments.  Never
 *     throws/aborts.  fd_last_error() describes the last failure on the calling thread.
 *   - reductions are deterministic (fixed trees, no float atomics).
 */
#ifndef FDHIP_H
#define FDHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: fd_tuning / fd_set_tuning added (the library no longer reads the process environment); fd_conv2d_fwd_stats and
 *    fd_bn_train_fwd_parts added, the fd_conv2d_*_pair entry points removed, fd_bn_ws_floats grew by one shift value per
 *    (group, channel) - a client that sized the BatchNorm workspace itself must re-query it.
 * 3: additions only (round 5): fd_masked_median, fd_refine_inputs (+ fd_refine_cfg), fd_resize_linear_cv, fd_bn_relu_maxpool_fwd / _bwd,
 *    fd_bn_train_bwd_remask, fd_stack_normalize, fd_conv2d_fwd_bn(_ok), fd_pose_head_fwd / _bwd; fd_tuning grew at its end
 *    (wino_min_cout, wino_wgrad_min_cout, wino_wgrad_xcd_few, wino_fwd_halfm, wino_wgrad_halfm, grp_tile64_below).  Nothing removed, no signature changed.
 * 4: additions only (round 6): fd_replay (+ fd_call_rec, fd_replay_function_count / _name / _signature); fd_tuning grew at its end (limb_1x1,
 *    limb_depth, limb_target, limb_split_max_out, limb_wgrad_target, limb_conv, wino_wgrad_limb, wino_fwd_limb); fd_relayout_job.mode 7 / 8 (1x1 weights pre-split into bf16
 *    limbs) and 9 / 10 (the same for a tap subset of a larger kernel); fd_refine_cfg accepts an empty crop window.  Nothing removed, no
 *    signature changed.
 * 5: additions only: graph-based depth correction (fd_gdc_prepare_ws_bytes, fd_gdc_prepare, fd_gdc_ws_bytes, fd_gdc_build,
 *    fd_gdc_cg_iters, fd_gdc_finish, struct fd_gdc_state).  Nothing removed, no signature changed.
 * 6: additions only: the image half of the KITTI loader (fd_resize_lanczos_u8_ws_bytes, fd_resize_lanczos_u8, fd_color_jitter_u8_ws_bytes,
 *    fd_color_jitter_u8_means_offset, fd_color_jitter_u8, fd_u8_to_planes, struct fd_jitter_desc).  Nothing removed, no signature changed.
 * 7: additions only: KITTI depth completion (fd_depth_png_keys + struct fd_depth_png_desc, fd_completion_ws_bytes, fd_completion_medians,
 *    fd_completion_errors).  Nothing removed, no signature changed.
 * 8: additions only: the batched Eigen-split scorer (fd_eigen_scores_ws_bytes, fd_eigen_scores, struct fd_eigen_desc).  Nothing
 *    removed, no signature changed.
 *    Added later WITHOUT raising the number: the KITTI 3-D detection depth export (fd_depth_export + struct fd_export_desc,
 *    fd_depth_quantize_u16).  Nothing removed, no signature changed: a client built against 8 runs unchanged, and one that wants the
 *    export looks the two symbols up (dlsym) instead of comparing the number, which tests/test_eigen_eval_cpu.py pins at 8.
 *    Likewise the all-scales loss for one or three source frames: fd_photo_ms_ws_floats / _fwd / _bwd accept cfg.base.NF 1..3
 *    (first shipped as a separate fd_photo_msn_* triple, since folded into these; calls with NF == 2 are unchanged).
 *    Likewise the training-time scorer (fd_val_scores_ws_bytes, fd_val_scores; it reuses struct fd_eigen_desc).
 *    Likewise the Completor's training-time scorer (fd_completion_val_scores_ws_bytes, fd_completion_val_scores).
 *    Likewise the per-class Eigen-split scorer (fd_eigen_class_scores_ws_bytes, fd_eigen_class_scores, fd_class_errors; it reuses
 *    struct fd_eigen_desc, and the workspace sizes of the three scorers above are what they were).
 *    Likewise the renderer of evaluate_depth --visualize (fd_vis_render_ws_bytes, fd_vis_render; it reuses struct fd_eigen_desc).
 *    Likewise the trainer's image summaries (fd_log_sheets_ws_bytes, fd_log_sheets, struct fd_log_tile, struct fd_log_cfg).
 *    Likewise the pseudo-LiDAR point clouds (fd_points_export_ws_bytes, fd_points_export, struct fd_points_calib; it reuses
 *    struct fd_export_desc).
 *    Likewise the PNG encoder (fd_png_enc_layout, fd_png_enc_filter, fd_png_enc_plan, fd_png_enc_emit, fd_png_enc_finish,
 *    fd_png_enc_block_rows, struct fd_png_enc_desc / _sizes / _block).
 *    Likewise the JPEG encoder (fd_jpeg_enc_quant_tables, fd_jpeg_enc_header, fd_jpeg_enc_layout, fd_jpeg_enc_encode,
 *    struct fd_jpeg_enc_desc / _sizes / _result). */
#define FD_ABI_VERSION 8

int fd_abi_version(void);
const char* fd_supported_arch(void); /* "gfx950" */
const char* fd_last_error(void);

/* ------------------------------------------------------------------ tuning ----------------------
 * Kernel-selection thresholds, process-wide.  The library NEVER reads the process environment: its behaviour - which kernel
 * family a convolution is routed to, and therefore what fd_*_wt_floats / fd_*_ws_floats return - is a function of the arguments
 * and of this struct alone.  The defaults are the measured best on MI355X and are in force from load on; the other values exist
 * for A/B timing and for tests that pin a kernel family.  fd_set_tuning copies the struct (fields beyond `size` bytes keep their
 * defaults); it must not race with calls in flight on other threads, and size queries made before the change do not apply after
 * it (a caller that changes the tuning re-queries its workspaces; fd_tuning_generation() counts the changes). */
typedef struct fd_tuning {
    int size;                     /* sizeof(fd_tuning) as the caller compiled it */
    int wino_fwd;                 /* 1   3x3 stride-1 forward / data gradient on the Winograd kernels (0: direct implicit GEMM) */
    int wino_wgrad;               /* 1   their weight gradient on the transposed Winograd kernel */
    int wino_fwd_2d_min;          /* 65536   F(2x2,3x3) forward / data gradient from Cin*Cout on (0: F(2,3) along x everywhere) */
    int wino_fwd_2dp_min_wgs;     /* 160 below that Cin*Cout: F(2x2,3x3) with all 16 components in ONE workgroup (k_conv_wino2p, no slabs) where
                                         the launch has at least this many 64x64 output tiles (0: never - F(2,3) along x as in rounds 1-3) */
    int wino_fwd_2dp_dma;         /* 1   ... with its activations on the direct-to-LDS path where W % 4 == 0 (0: register-staged loader) */
    int wino_fwd_2dp_deep;        /* 0   1: the one-workgroup kernel also above wino_fwd_2d_min when the launch has enough tiles (A/B) */
    int wino_wgrad_2d;            /* 2   weight gradient as transposed F(2x2,3x3) where the height is even (1: and Cin % 32 == 0; 0: never) */
    int wino_target;              /* 384 workgroups a Winograd forward launch is split-K'd up to */
    int wino_wgrad_target;        /* 256 ... a Winograd weight-gradient launch is pixel-sliced up to */
    int conv_target;              /* 768 ... a direct forward / data-gradient launch */
    int wgrad_target;             /* 768 ... a direct weight-gradient launch */
    int conv_c1;                  /* 1   Cout == 1 layers (dispconv) as stencils (conv_c1.hip) */
    int conv_n16_min_pixels;      /* 16384   16 / 32-channel 3x3 blocks on k_conv3x3_n16 from this plane size on (< 0: never) */
    int reflect_ring;             /* 1   reflect-padded data gradients as interior + ring from 16384 pixels on (n > 1: from n pixels
                                         on; 0: always through the padded-grid tensor + fold pass) */
    int reflect_wino;             /* 1   the interior of such a gradient on the Winograd kernels (>= 64 input channels) */
    int reflect_wino_min_pixels;  /* 1   ... on planes of at least this many pixels */
    int reflect_wino_padded_max;  /* 4096   below this plane size: ONE Winograd convolution over the zero-bordered dY + fold (0: never) */
    int force_cfg, force_splits;  /* -1, 1   force the direct kernel's tile configuration (0..2) and split-K (sweeps) */
    int stem7;                    /* 1   7x7 stride-2 stems (Cin 2..6) on the dedicated patch kernels (conv_stem.hip) */
    int log;                      /* 0   1: one stderr line per convolution call with the kernel family it was routed to */
    int wino_fwd_2d_m128;         /* 1   the slab variant with 128 output channels per workgroup (k_conv_wino2d_m128) wherever it can run (Cout % 128 == 0, W % 4 == 0); 2: only where its launch fills the chip better; 0: never */
    int wino_min_cout;            /* 32  fewest output channels of a forward / data-gradient launch on the Winograd kernels (their tile is 64 channels
                                         tall: below that, rows of the tile are idle; 32 = the depth decoder's upconv(1, *) as well; rounds 1-4: 64) */
    int wino_wgrad_min_cout;      /* 32  ... of a weight-gradient launch */
    int wino_wgrad_xcd_few;       /* 1   Winograd weight gradients with 2 or 4 pixel slices on the XCD-aware grid as well (each slice owns 4 / 2 XCDs) */
    int wino_fwd_halfm;           /* 1   k_conv_wino2p_dma with <= 32 output channels likewise (forward of the decoder's upconv(1, *)) */
    int wino_wgrad_halfm;         /* 1   Winograd weight gradients with <= 32 output channels: the tile's idle wave pair takes half of every chunk's K-steps */
    int grp_tile64_below;         /* 0   grouped launches (the four parity classes of a stride-2 data gradient) with fewer than this many 64x128
                                         workgroups run on 64x64 tiles (twice the workgroups, half the work of the longest one); 0: never */
    int limb_1x1;                 /* 1   1x1 stride-1 convolutions with >= 64 channels on both sides (ResNet-50 bottlenecks) as split-precision GEMMs on the
                                         bf16 MFMA: every fp32 operand = 3 bf16 limbs, six limb products, fp32 accumulation - fp32 accuracy
                                         (csrc/conv_limb.hip); 0: the f32-MFMA direct kernels */
    int limb_depth;               /* 2   K-chunks (16 channels each) of operands a thread of the limb GEMMs keeps in flight (2 or 4) */
    int limb_target;              /* 256 workgroups a limb forward / data-gradient launch is split-K'd up to ... */
    int limb_split_max_out;       /* 4194304   ... when its output has at most this many floats (a split costs a slab round trip of the output) */
    int limb_wgrad_target;        /* 256 workgroups a limb weight-gradient launch is pixel-sliced up to (x2 for its 4-wave tiles) */
    int limb_conv;                /* 1   stride-2 convolutions with >= 64 channels on both sides (ResNet layerN.0.conv1 / downsample: no Winograd form), forward
                                         and data gradient, as split-precision implicit GEMMs (k_conv_limb); 0: the f32-MFMA direct kernels */
    int wino_wgrad_limb;          /* 2   the 2-D Winograd weight gradient with >= 64 output channels and W % 8 == 0 with a split-precision matrix loop
                                         (k_wgrad_wino_limb: transforms + limb split in the loader, 768 instead of 2 048 matrix cycles per chunk): 1 the
                                         zero-padded layers (ResNet trunk), 2 the reflect-padded decoder blocks as well, 0 the f32 kernel everywhere */
    int wino_fwd_limb;            /* 0   1: the F(2x2, 3x3) slab kernel of the deep layers (forward / data gradient, >= 64 channels on both sides, W % 4 == 0)
                                         with pre-split weights and a split-precision matrix loop (k_conv_wino2d_limb) instead of k_conv_wino2d(_m128).
                                         Per-kernel error vs float64 equal to the f32 kernels' and +0.2 ... +0.8 % in the step, but OFF: with it one bound
                                         of the full-size backward test at 1024x320 is exceeded (depth-decoder gradient norm 1.81e-3 against 1.65e-3) */
} fd_tuning;
void fd_tuning_defaults(fd_tuning* t);
int fd_set_tuning(const fd_tuning* t);
void fd_get_tuning(fd_tuning* t);
long fd_tuning_generation(void);

/* ------------------------------------------------------------------ geometry (layers.py) ------- */

/* layers.py:11-20 disp_to_depth.  depth and/or scaled may be NULL. */
int fd_disp_to_depth_fwd(const float* disp, float* scaled, float* depth, long n, double min_depth, double max_depth,
                         void* stream);
/* d_disp = g_scaled*(max_disp-min_disp) - g_depth*(max_disp-min_disp)*depth^2 ; either g may be NULL */
int fd_disp_to_depth_bwd(const float* disp, const float* g_scaled, const float* g_depth, float* d_disp, long n,
                         double min_depth, double max_depth, void* stream);

/* layers.py:23-97 transformation_from_parameters (+rot_from_axisangle, get_translation_matrix).
 * axisangle, translation: [B,3]; T: [B,4,4].  invert: M = R^T * T(-t), else T(t) * R. */
int fd_pose_matrix_fwd(const float* axisangle, const float* translation, float* T, int B, int invert, void* stream);
int fd_pose_matrix_bwd(const float* axisangle, const float* translation, const float* gT, float* g_axisangle,
                       float* g_translation, int B, int invert, void* stream);

/* trainer.py:338-360 for the STACKED pose network (all frame pairs x accumulated micro-batches in one batch): pose [G*nf*Bq][ld] = the
 * pose decoder's output (networks/pose_decoder.py:47-51: 0.01 * mean, ld = 6 * predictions; prediction 0 = columns 0..5 is the one
 * trainer.py:350-352 uses), rows ordered (micro-batch g, frame pair k, sample s) -> per frame pair k: T[k] [G*Bq][4][4] (bit k of
 * invert_mask: trainer.py:352 invert=(f_i < 0)) and, if given, axisangle[k] / translation[k] [G*Bq][ld/6][3] (the outputs dictionary's
 * entries).  T / axisangle / translation / gT: HOST arrays of nf (<= 4) device pointers.  Replaces, per frame pair, the slicing +
 * concatenation + fd_pose_matrix_fwd / _bwd launches (and autograd's ~20 element-wise launches per pair behind them).
 * bwd: g_pose [G*nf*Bq][ld], fully written (unused predictions: 0); gT[k] == NULL: that matrix received no gradient. */
int fd_pose_head_fwd(const float* pose, float* const* T, float* const* axisangle, float* const* translation, int G, int nf, int Bq,
                     int ld, unsigned invert_mask, void* stream);
int fd_pose_head_bwd(const float* pose, const float* const* gT, float* g_pose, int G, int nf, int Bq, int ld, unsigned invert_mask,
                     void* stream);

/* layers.py:217 `P = matmul(K, T)[:, :3, :]`.  K,T: [B,4,4]; P: [B,3,4] written at P + b*p_batch_stride. */
int fd_proj_matrix_fwd(const float* K, const float* T, float* P, long p_batch_stride, int B, void* stream);
/* gT[B,4,4] = K[:3,:]^T * gP */
int fd_proj_matrix_bwd(const float* K, const float* gP, long p_batch_stride, float* gT, int B, void* stream);

/* layers.py:157-162 BackprojectDepth.forward: depth[B,1,H,W], inv_K[B,4,4] -> points [B,4,H*W]. */
int fd_backproject_fwd(const float* depth, const float* inv_K, float* points, int B, int H, int W, void* stream);
int fd_backproject_bwd(const float* g_points, const float* inv_K, float* g_depth, int B, int H, int W, void* stream);

/* layers.py:215-226 Project3D.forward: points[B,4,H*W], K, T -> grid [B,H,W,2]. */
int fd_project3d_fwd(const float* points, const float* K, const float* T, float* grid, int B, int H, int W, float eps,
                     void* stream);
/* g_points [B,4,HW] (row 3 gets its true gradient too); gP partial sums need `ws` of
 * fd_project3d_bwd_ws_floats(B,H,W) floats; gT [B,4,4]. */
long fd_project3d_bwd_ws_floats(int B, int H, int W);
int fd_project3d_bwd(const float* points, const float* K, const float* T, const float* g_grid, float* g_points,
                     float* gT, float* ws, int B, int H, int W, float eps, void* stream);

/* layers.py:187-201 Cat_xy.forward (refiner.py input channels). out [B,3,H,W]. */
int fd_cat_xy_fwd(const float* depth, const float* inv_K, float* out, int B, int H, int W, void* stream);

/* F.interpolate(x,[Hout,Wout],mode="bilinear",align_corners=False) (trainer.py:434-435,:579) on BC = B*C planes, 0 < BC < 65536.
 * _fwd takes any sizes (ATen's rule, no antialiasing).  _bwd is its adjoint for Hout >= Hin and Wout >= Win only, at any ratio,
 * integer or fractional, the two axes independently; anything smaller is refused (non-zero return, gx not written). */
int fd_bilinear_up_fwd(const float* x, float* y, int BC, int Hin, int Win, int Hout, int Wout, void* stream);
int fd_bilinear_up_bwd(const float* gy, float* gx, int BC, int Hin, int Win, int Hout, int Wout, void* stream);

/* ------------------------------------------------------------------ photometric loss ----------- */

/* layers.py:267-281 SSIM.forward -> out [B,C,H,W] = clamp((1-SSIM)/2,0,1). */
int fd_ssim_fwd(const float* x, const float* y, float* out, int B, int C, int H, int W, void* stream);
/* gradients of sum(out*g) w.r.t. x and y (either may be NULL). */
int fd_ssim_bwd(const float* x, const float* y, const float* g, float* gx, float* gy, int B, int C, int H, int W,
                void* stream);

/* trainer.py:476-488 compute_reprojection_loss (3-channel images): out[b] at out + b*out_batch_stride,
 * = 0.85*mean_c SSIM + 0.15*mean_c|t-p|  (use_ssim) or mean_c|t-p|. */
int fd_reproj_loss_map(const float* pred, const float* target, float* out, long out_batch_stride, int B, int H, int W,
                       int use_ssim, void* stream);

/* Fused per-scale photometric + LiDAR loss, forward.  Replaces, for one scale, trainer.py:434-470
 * (bilinear upsample of disp, disp_to_depth, BackprojectDepth, Project3D, F.grid_sample(border)) and
 * trainer.py:509-567,577-589 (SSIM+L1 reprojection losses, identity losses + noise, per-pixel min,
 * mean; masked scale-invariant log loss vs the 4-beam LiDAR).
 *
 *   disp      [B,1,Hs,Ws]   sigmoid output of the decoder at this scale
 *   inv_K     [B,4,4]       inverse intrinsics at the sampling resolution (H,W)
 *   P         [B,NF,3,4]    (K @ cam_T_cam_f)[:3] per source frame (fd_proj_matrix_fwd)
 *   src       NF pointers   source colour images [B,3,H,W]
 *   target    [B,3,H,W]
 *   ident     [B,NI,H,W]    identity reprojection losses (NI = NF, or 1 if avg_reprojection) or NULL
 *   noise     [B,NI,H,W]    tie-break noise (scaled by 1e-5 inside) or NULL
 *   beam      [B,1,H,W]     4-beam LiDAR depth / 100, or NULL to skip the SI loss
 *   sel       [B,H,W] u8    out: argmin index into cat(ident, reproj) (trainer.py:561)
 *   depth_out/sample_out/color_out   optional materialised ("depth",0,s) [B,1,H,W],
 *                           ("sample",f,s) [NF][B,H,W,2], ("color",f,s) [NF][B,3,H,W]  (NULL to skip)
 *   ws        workspace of fd_photo_ws_floats(B,H,W) floats (per-block partial sums)
 *   out       [FD_PHOTO_OUT_FLOATS] floats: 0 to_optimise.mean() over the whole batch, 4 si_loss averaged over the
 *             `groups` sub-batches, 8+4g.. per group g: n_valid, mean(d), mean(d^2)-si_var*mean(d)^2, si_loss_g
 *             (1..3 repeat group 0; the rest is scratch)
 *   cfg.groups  G >= 1: the batch is G stacked micro-batches (trainer.py:237-248 accumulates their losses); the SI-log
 *             loss, which is not linear in the batch, is evaluated per micro-batch and averaged.
 */
#define FD_PHOTO_OUT_FLOATS 96
typedef struct {
    double min_depth, max_depth; /* opt.min_depth / opt.max_depth (doubles: 1/0.1 must be exactly 10) */
    int B, H, W, Hs, Ws, NF;
    int use_ssim;        /* !opt.no_ssim */
    int avg_reprojection;
    float si_depth_scale;   /* 26.0  (trainer.py:583) */
    float si_beam_scale;    /* 100.0 (trainer.py:581) */
    float si_threshold;     /* opt.gdc_loss_threshold */
    float si_var;           /* opt.si_var */
    float eps;              /* Project3D eps 1e-7 */
    int groups;             /* number of stacked micro-batches (>= 1) */
    float si_lo;            /* lower bound of the SI-loss mask: target > si_lo && pred > si_lo  (1.0 in trainer.py:584-586,
                               1e-3 in refiner.py:561-562) */
    int si_mode;            /* LiDAR term: 0 = scale-invariant log loss * 0.1 (trainer.py:577-589, completor.py:699-716),
                               1 = masked L1 * 0.001 without the |pred - beam| gate (completor.py:718-723, --completion_l1loss);
                               out[8+4g+1] then holds mean |pred - beam| */
} fd_photo_cfg;

long fd_photo_ws_floats(int B, int H, int W);
int fd_photo_fwd(const fd_photo_cfg* cfg, const float* disp, const float* inv_K, const float* P,
                 const float* const* src, const float* target, const float* ident, const float* noise,
                 const float* beam, uint8_t* sel, float* depth_out, float* sample_out, float* color_out, float* ws,
                 float* out, void* stream);
/* Backward of the above.  g [2] device floats: dL/d(out[0]), dL/d(out[4]).  stats = `out` of the
 * forward; has_ident = whether the forward was given `ident` (needed to decode `sel`).
 * d_disp [B,1,Hs,Ws]; gP [B,NF,3,4]; ws: fd_photo_bwd_ws_floats(B,H,W) floats. */
long fd_photo_bwd_ws_floats(int B, int H, int W);
int fd_photo_bwd(const fd_photo_cfg* cfg, const float* disp, const float* inv_K, const float* P,
                 const float* const* src, const float* target, const float* beam, const uint8_t* sel, int has_ident,
                 const float* stats, const float* g, float* d_disp, float* gP, float* ws, void* stream);
/* The same pair with the remaining flag variants of trainer.py:425-567: up to THREE source frames (--use_stereo adds the
 * stereo partner "s" to frames -1 / +1, trainer.py:436-439) and the predictive-mask baseline (--predictive_mask,
 * trainer.py:117-127, 530-541).
 *   mask        [B,NF,H,W] or NULL: the reprojection loss of frame f is multiplied by mask[:, f] before the minimum /
 *               average (the mask replaces automasking: `ident` must be NULL when it is given)
 *   reproj_out  [B,NF,H,W] or NULL: the UNmasked reprojection losses; d out[0] / d mask[:, f] = reproj_out[:, f] / (B H W)
 *               where frame f was selected (`sel`), or / NF everywhere with avg_reprojection - the caller forms it.
 * fd_photo_fwd / fd_photo_bwd are these with mask = reproj_out = NULL. */
int fd_photo_fwd_ex(const fd_photo_cfg* cfg, const float* disp, const float* inv_K, const float* P,
                    const float* const* src, const float* target, const float* ident, const float* noise,
                    const float* beam, const float* mask, uint8_t* sel, float* depth_out, float* sample_out,
                    float* color_out, float* reproj_out, float* ws, float* out, void* stream);
int fd_photo_bwd_ex(const fd_photo_cfg* cfg, const float* disp, const float* inv_K, const float* P,
                    const float* const* src, const float* target, const float* beam, const float* mask, const uint8_t* sel,
                    int has_ident, const float* stats, const float* g, float* d_disp, float* gP, float* ws, void* stream);

/* ---- all pyramid scales in one launch, value + unit-cotangent gradient in the same pass ------------------------------
 * Replaces the per-scale loop of trainer.py:425-474 (generate_images_pred) + trainer.py:509-567, 577-589 (compute_losses)
 * for the default configuration: SSIM + L1, per-frame minimum (automasking on or off), SI-log or masked L1 LiDAR term on any
 * subset of the scales, and NF = 1 to 3 source frames: two by default; --use_stereo makes it one (frame_ids [0, "s"]) or three
 * ([0, -1, 1, "s"]), the stereo partner's pose being just one more P.  One wave per source frame and strip
 * (csrc/photometric_ms.hip).  The flag variants (--no_ssim, --avg_reprojection, the materialised ("depth"|"sample"|"color", f, s)
 * outputs) stay on fd_photo_fwd / fd_photo_bwd.
 *   cfg.base      as for fd_photo_fwd (Hs / Ws ignored: per-scale sizes are cfg.Hs[] / cfg.Ws[]); NF must be 1, 2 or 3
 *   src[NF]       [B,3,H,W] each         P         [B,NF,3,4]
 *   disp[s]       [B,1,Hs[s],Ws[s]]      noise[s]  [B,NF,H,W] or NULL (the array itself may be NULL)
 *   ident         [B,NF,H,W] or NULL     beam      [B,1,H,W] or NULL; cfg.beam_mask bit s = scale s carries the LiDAR term
 *   sel           [S,B,H,W] u8 out: index into cat(ident_0.., reproj_0..) (0 .. 2 NF - 1; 0 .. NF - 1 without ident)
 *   d1            [S,B,H,W] out: d out[s][0] / d disp_up, or NULL to skip every gradient
 *   ws            fd_photo_ms_ws_floats(cfg) floats; must stay untouched until fd_photo_ms_bwd has run
 *   out           [S][FD_PHOTO_OUT_FLOATS], each laid out like fd_photo_fwd's `out`
 * fd_photo_ms_bwd: g_photo[s] / g_si[s] = device pointers to dL/d out[s][0] / dL/d out[s][4] (NULL = 0); d1 is read only;
 * d_disp[s] [B,1,Hs[s],Ws[s]] out (H / Hs[s] == W / Ws[s] must be an integer <= 16);
 * gP [B,NF,3,4] out = sum over scales of g_photo[s] * d out[s][0] / d P. */
typedef struct {
    fd_photo_cfg base;
    int n_scales;            /* 1..4 */
    int Hs[4], Ws[4];
    unsigned beam_mask;
    int rows_per_strip;      /* image rows a wave streams through; 0 = default */
} fd_photo_ms_cfg;
long fd_photo_ms_ws_floats(const fd_photo_ms_cfg* cfg);
int fd_photo_ms_fwd(const fd_photo_ms_cfg* cfg, const float* const* disp, const float* inv_K, const float* P,
                    const float* const* src, const float* target, const float* ident, const float* const* noise,
                    const float* beam, uint8_t* sel, float* d1, float* ws, float* out, void* stream);
int fd_photo_ms_bwd(const fd_photo_ms_cfg* cfg, const float* const* disp, const float* beam, const float* stats,
                    const float* const* g_photo, const float* const* g_si, float* d1, const float* ws,
                    float* const* d_disp, float* gP, void* stream);

/* layers.py:235-248 get_smooth_loss on the mean-normalised disparity (trainer.py:569-571):
 * out[0] = get_smooth_loss(disp/(mean_hw(disp)+1e-7), img).  ws: fd_smooth_ws_floats(B,H,W). */
long fd_smooth_ws_floats(int B, int H, int W);
int fd_smooth_fwd(const float* disp, const float* img, float* out, float* ws, int B, int H, int W, int normalize,
                  void* stream);
/* d_disp [B,1,H,W] = g[0] * d out[0] / d disp */
int fd_smooth_bwd(const float* disp, const float* img, const float* g, float* d_disp, float* ws, int B, int H, int W,
                  int normalize, void* stream);

/* ------------------------------------------------------------------ convolution stack ---------- */

/* One 2-D convolution, NCHW fp32, square kernel 1/3/5/7, stride 1|2, symmetric padding.
 * Replaces nn.Conv2d / layers.Conv3x3 / layers.ConvBlock call sites:
 *   networks/resnet_encoder.py:95,98-101 (torchvision ResNet convs, zero pad, no bias),
 *   layers.py:115-130 (ReflectionPad2d(1)+Conv2d 3x3 + bias), layers.py:100-112 (+ELU),
 *   networks/depth_decoder.py:92 (dispconv + sigmoid), networks/pose_decoder.py:35-42 (+ReLU). */
typedef struct {
    int N, Cin, H, W;       /* input  [N,Cin,H,W]                    */
    int Cout, KH, KW;       /* weight [Cout,Cin,KH,KW] (OIHW)        */
    int stride, pad;
    int pad_mode;           /* 0 zero, 1 reflect (stride 1, pad 1)   */
    int act;                /* epilogue: 0 none, 1 ReLU, 2 ELU, 3 sigmoid, 4 tanh (applied after bias) */
    int in_norm;            /* 1: taps read (x-0.45)/0.225 (resnet_encoder.py:94), padding stays 0 */
} fd_conv_desc;

/* y [N,Cout,Ho,Wo] = act(conv(x, w) + bias);  bias may be NULL.
 *   wt  caller-owned buffer of fd_conv2d_fwd_wt_floats(d) floats holding the kernel's weight layout ([Cout][tap][Cin]);
 *       it is (re)written from `w` unless wt_ready != 0, so a caller may keep it across calls while `w` is unchanged
 *       (the trainer re-derives it once per optimiser step).  May be NULL when the size query returns 0.
 *   ws  scratch of fd_conv2d_fwd_ws_floats(d) floats (split-K slabs; may be 0 -> NULL). */
long fd_conv2d_fwd_wt_floats(const fd_conv_desc* d);
long fd_conv2d_fwd_ws_floats(const fd_conv_desc* d);
int fd_conv2d_fwd(const fd_conv_desc* d, const float* x, const float* w, const float* bias, float* y, float* wt,
                  int wt_ready, float* ws, void* stream);
/* BatchNorm statistics from the convolution's own epilogue.  Every ResNet convolution is followed by a training-mode BatchNorm
 * (networks/resnet_encoder.py:95-101 -> torchvision BasicBlock / Bottleneck), whose first pass - per-channel sum and sum of
 * squares of the convolution output - the convolution kernel can produce while the output tile is still in registers:
 *   fd_conv2d_fwd_stat_slots  S = partial-sum slots per (image, output channel) the kernel chosen for `d` writes, or 0 when that
 *                             kernel has no statistics epilogue (split-K launches, tiles that straddle images, fused activations):
 *                             the caller then uses fd_bn_train_fwd, which makes its own statistics pass.
 *   fd_conv2d_fwd_stats       fd_conv2d_fwd that also fills part [N][Cout][S][2] = (sum, M2) of y per slot of H*W/S pixels,
 *                             M2 = sum of squared deviations from the slot's own mean (merged without cancellation).
 *   fd_bn_train_fwd_parts     fd_bn_train_fwd (same semantics: per-group statistics, running statistics updated in group order)
 *                             with the statistics taken from such partial sums - one launch, one pass over x less. */
long fd_conv2d_fwd_stat_slots(const fd_conv_desc* d);
int fd_conv2d_fwd_stats(const fd_conv_desc* d, const float* x, const float* w, const float* bias, float* y, float* wt,
                        int wt_ready, float* ws, float* stat_part, void* stream);
int fd_bn_train_fwd_parts(const float* x, const float* weight, const float* bias, const float* residual, float* y,
                          float* running_mean, float* running_var, float* save_mean, float* save_invstd, const float* conv_part,
                          int slots, int N, int C, int H, int W, int groups, float eps, float momentum, int relu, void* stream);

/* Batched weight re-layout.  A training step re-derives the kernel-side copy of every conv weight once per optimiser
 * step; instead of one small launch per convolution inside fd_conv2d_fwd / fd_conv2d_bwd_data (wt_ready = 0) the caller can
 * collect the work of all its convolutions once and run it as ONE launch after each optimiser update, then call the
 * convolutions with wt_ready = 1.
 *   fd_conv2d_relayout_jobs  appends to jobs[] (capacity >= 4) what the forward (kind 0) or data-gradient (kind 1) of `d`
 *                            would re-lay-out from `w` into `wt`; returns the number of jobs (0: that path needs no copy).
 *   fd_relayout_plan         fills the launch bookkeeping of a host array of n jobs; returns the workgroup count.
 *   fd_relayout_batch        runs n jobs; `jobs_dev` is the planned array copied to DEVICE memory. */
typedef struct fd_relayout_job {
    const float* w;
    float* dst;
    int Co, Ci, KH, KW, TA, TB, kh0, dkh, kw0, dkw;
    int mode;          /* 0 forward [Co][tap][Ci], 1 data-gradient [Ci][tap][Co], 2 generic data-gradient [Ci][Co][tap]; 3 - 6 Winograd U;
                          7 / 8 the 1x1 matrix, 9 / 10 the [m][(tap, channel)] matrix of layouts 0 / 1 pre-split into bf16 limbs (csrc/conv_limb.h); 11 / 12 the limb image of layouts 5 / 6 */
    int reserved;
    long n;            /* elements */
    long first_block;  /* set by fd_relayout_plan */
} fd_relayout_job;
int fd_conv2d_relayout_jobs(const fd_conv_desc* d, int kind, const float* w, float* wt, fd_relayout_job* jobs);
long fd_relayout_plan(fd_relayout_job* jobs_host, int n);
int fd_relayout_batch(const fd_relayout_job* jobs_dev, int n, long total_blocks, void* stream);

/* gx [N,Cin,H,W] = d/dx of sum(conv(x,w) * gy)  (gy is the gradient w.r.t. the PRE-activation output;
 * apply fd_act_bwd first when act != 0).  wt / wt_ready as in fd_conv2d_fwd (flipped / transposed layouts, one per
 * output-parity class for stride 2: fd_conv2d_bwd_data_wt_floats(d) floats); ws: fd_conv2d_bwd_data_ws_floats(d). */
long fd_conv2d_bwd_data_wt_floats(const fd_conv_desc* d);
long fd_conv2d_bwd_data_ws_floats(const fd_conv_desc* d);
int fd_conv2d_bwd_data(const fd_conv_desc* d, const float* gy, const float* w, float* gx, float* wt, int wt_ready, float* ws,
                       void* stream);
/* gx = (data gradient as above) + gx_add, gx_add [N,Cin,H,W] (must not alias gx): where a tensor feeds a convolution AND a second
 * consumer - the input of a ResNet block also is its residual branch (torchvision BasicBlock / Bottleneck `out += identity`, used
 * by networks/resnet_encoder.py:61-75) - autograd has to sum two gradients; here the second one joins in the epilogue of the
 * data-gradient kernel instead of costing an element-wise pass over both tensors.  Bitwise the sum torch would form. */
int fd_conv2d_bwd_data_add(const fd_conv_desc* d, const float* gy, const float* w, const float* gx_add, float* gx, float* wt,
                           int wt_ready, float* ws, void* stream);
/* gx = (data gradient as above) * act'(x_in): for a layer whose INPUT x_in is the output of activation in_act (1 ReLU, 2 ELU, 3 sigmoid,
 * 4 tanh) and is consumed by this layer alone, the result is the gradient w.r.t. the producer's PRE-activation - what fd_act_bwd
 * would compute from gx in a separate pass over the tensor (layers.py:100-112 ConvBlock -> networks/depth_decoder.py:92 dispconv:
 * the full-resolution ELU output feeds the disparity head only).  Fused into the store of the one-output-channel stencil; the other
 * kernel families run the data gradient followed by the element-wise pass (same result). */
int fd_conv2d_bwd_data_inact(const fd_conv_desc* d, const float* gy, const float* w, const float* x_in, int in_act, float* gx, float* wt,
                             int wt_ready, float* ws, void* stream);
/* gw [Cout,Cin,KH,KW], gbias [Cout] (NULL to skip).  accumulate != 0: gw += / gbias += (gradient accumulation straight
 * into the caller's buffers).  ws: fd_conv2d_bwd_weight_ws_floats(d) floats. */
long fd_conv2d_bwd_weight_ws_floats(const fd_conv_desc* d);
int fd_conv2d_bwd_weight(const fd_conv_desc* d, const float* x, const float* gy, float* gw, float* gbias, float* ws,
                         int accumulate, void* stream);

/* gpre = gy * act'(y)  where y is the activation OUTPUT (1 ReLU, 2 ELU(alpha=1), 3 sigmoid, 4 tanh). */
/* Convolution + training-mode BatchNorm (+ residual, ReLU) of a deep ResNet block in two launches (round 5): for the 3x3 layers that
 * run as F(2x2, 3x3) slabs (layer3 / layer4) the slab reduction of the convolution happens inside the small-plane BatchNorm kernel.
 * fd_conv2d_fwd_bn_ok(d, groups) == 1 says that this convolution (no bias, no activation) + BatchNorm qualifies; then
 * fd_conv2d_fwd_bn == fd_conv2d_fwd(d, x, w, NULL, y, wt, wt_ready, ws) followed by fd_bn_train_fwd(y, ..., out, ...): same y bit
 * for bit, same statistics rule as the small-plane kernel.  ws / wt as for fd_conv2d_fwd. */
int fd_conv2d_fwd_bn_ok(const fd_conv_desc* d, int groups);
int fd_conv2d_fwd_bn(const fd_conv_desc* d, const float* x, const float* w, float* y, float* wt, int wt_ready, float* ws,
                     const float* bn_weight, const float* bn_bias, const float* residual, float* out, float* running_mean,
                     float* running_var, float* save_mean, float* save_invstd, int groups, float eps, float momentum, int relu,
                     void* stream);
int fd_act_bwd(const float* y, const float* gy, float* gpre, long n, int act, void* stream);

/* nn.BatchNorm2d in training mode (torchvision ResNet; trainer.py:207-211 set_train), optionally fused with the
 * residual add and ReLU of a BasicBlock/Bottleneck tail:  y = relu?( bn(x) + residual? ).
 * `groups` G >= 1 splits the batch into G consecutive sub-batches that are normalised independently — bit-for-bit what G
 * separate forward passes would do (predict_poses runs the pose encoders once per source frame, trainer.py:336-351; the
 * trainer batches those passes) — including G in-order momentum updates of the running statistics.
 * save_mean / save_invstd [G*C] are written for the backward; running_mean / running_var are updated in place
 * with `momentum` (unbiased variance), as torch does.  ws: fd_bn_ws_floats(N,C,H,W,G).
 * Non-finite input: a NaN or an infinity in a (group, channel) makes that channel's y, save_invstd and running_var NaN (the mean
 * of a channel with an infinity is that infinity), with or without the ReLU, as torch does; other channels are untouched.
 * Every fd_bn_* entry point that launches one grid row per (sample, channel) plane refuses N * C > 65535 (status -1). */
long fd_bn_ws_floats(int N, int C, int H, int W, int groups);
int fd_bn_train_fwd(const float* x, const float* weight, const float* bias, const float* residual, float* y,
                    float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* ws, int N, int C,
                    int H, int W, int groups, float eps, float momentum, int relu, void* stream);
/* eval-mode BN (running statistics), same fusion options. */
int fd_bn_eval_fwd(const float* x, const float* weight, const float* bias, const float* residual, float* y,
                   const float* running_mean, const float* running_var, int N, int C, int H, int W, float eps, int relu,
                   void* stream);
/* Backward of the fused op.  y = forward output (for the ReLU mask when relu=1).  gx, gweight, gbias are
 * written; g_residual (if non-NULL) receives the masked upstream gradient (the residual branch's gradient). */
int fd_bn_train_bwd(const float* x, const float* y, const float* gy, const float* weight, const float* save_mean,
                    const float* save_invstd, float* gx, float* gweight, float* gbias, float* g_residual, float* ws, int N,
                    int C, int H, int W, int groups, int relu, int accumulate /* gweight/gbias += */, void* stream);

/* The same backward for a BatchNorm + ReLU WITHOUT a residual input (bn1 of a BasicBlock, bn1 / bn2 of a Bottleneck): the ReLU mask
 * is recomputed from x (weight * invstd * (x - mean) + bias > 0), so the forward output is not read - two tensors per pass instead
 * of three (round 5). */
int fd_bn_train_bwd_remask(const float* x, const float* gy, const float* weight, const float* bias, const float* save_mean,
                           const float* save_invstd, float* gx, float* gweight, float* gbias, float* ws, int N, int C, int H, int W,
                           int groups, int accumulate, void* stream);

/* nn.MaxPool2d(3, stride 2, padding 1) (resnet_encoder.py:98).  idx [N,C,Ho,Wo] u8 = argmax tap (0..8). */
int fd_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int C, int H, int W, void* stream);
int fd_maxpool3x3s2_bwd(const float* gy, const uint8_t* idx, float* gx, int N, int C, int H, int W, void* stream);

/* The stem's tail in one pass (resnet_encoder.py:95-98: features[0] = relu(bn1(conv1(x))), x = maxpool(features[0])), training mode:
 * fd_bn_train_fwd(relu = 1) + fd_maxpool3x3s2_fwd without the round trip of the full-resolution activation through memory.
 *   fwd  x [N,C,H,W] (the convolution's output) -> pooled [N,C,Ho,Wo], idx (argmax tap, u8), and - only when feat != NULL - feat
 *        [N,C,H,W] = relu(bn(x)) (the encoders whose features[0] nobody reads, the pose encoders, pass NULL); statistics, groups,
 *        running statistics, save_mean / save_invstd and ws exactly as fd_bn_train_fwd.
 *   bwd  g_pooled (+ g_feat, the gradient arriving at features[0] from its other consumer, or NULL) -> gx [N,C,H,W], gweight, gbias:
 *        the ReLU mask and the normalised value are recomputed from x, the pooling adjoint from g_pooled and idx. */
int fd_bn_relu_maxpool_fwd(const float* x, const float* weight, const float* bias, float* feat, float* pooled, uint8_t* idx,
                           float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* ws, int N, int C, int H,
                           int W, int groups, float eps, float momentum, void* stream);
int fd_bn_relu_maxpool_bwd(const float* x, const float* g_pooled, const uint8_t* idx, const float* g_feat, const float* weight,
                           const float* bias, const float* save_mean, const float* save_invstd, float* gx, float* gweight, float* gbias,
                           float* ws, int N, int C, int H, int W, int groups, int accumulate, void* stream);

/* Decoder input assembly (networks/depth_decoder.py:75-83): out = cat([nearest_up2(a), s1 (+ s2), s3], dim=1).
 * a [N,Ca,h,w] -> channels [0,Ca) at (2h,2w); s1,s2 [N,Cs,2h,2w] (s2 optional addend: beam-feature fusion
 * depth_decoder.py:78); s3 [N,C3,2h,2w] optional (refiner depth_maps, :81-82).  Any of s1/s3 may be NULL. */
int fd_upcat_fwd(const float* a, const float* s1, const float* s2, const float* s3, float* out, int N, int Ca, int Cs,
                 int C3, int h, int w, void* stream);
/* ga [N,Ca,h,w] (2x2 sums), gs [N,Cs,2h,2w] (shared by s1 and s2), g3 [N,C3,2h,2w]; each may be NULL. */
int fd_upcat_bwd(const float* gout, float* ga, float* gs, float* g3, int N, int Ca, int Cs, int C3, int h, int w,
                 void* stream);
/* The same with ga *= act'(a_out): `a` was the output of activation a_act (layers.py:100-112 ConvBlock, upconv(i, 0)) and feeds this
 * concatenation only, so ga is the gradient w.r.t. that layer's PRE-activation (no separate fd_act_bwd pass). */
int fd_upcat_bwd_act(const float* gout, const float* a_out, int a_act, float* ga, float* gs, float* g3, int N, int Ca, int Cs, int C3,
                     int h, int w, void* stream);
/* layers.py:229-232 upsample (nearest x2) alone */
int fd_upsample2x_fwd(const float* x, float* y, long planes, int h, int w, void* stream);
int fd_upsample2x_bwd(const float* gy, float* gx, long planes, int h, int w, void* stream);

/* trainer.py:569-596  loss_s = photo_s + w * smooth_s / 2^s ;  total = (sum_s loss_s + sum_s si_s) / n_scales  on device
 * scalars (photo / smooth / si: n_scales host arrays of device pointers to one float; si[s] may be NULL).
 * out[0..n-1] = loss_s, out[n] = total.  bwd: grads[0..n-1] = d total/d photo_s, [n..2n-1] = d/d smooth_s, [2n..3n-1] = d/d si_s. */
int fd_combine_losses_fwd(const float* const* photo, const float* const* smooth, const float* const* si, int n_scales,
                          float smooth_weight, float* out, void* stream);
int fd_combine_losses_bwd(const float* g_total, int n_scales, float smooth_weight, float* grads, void* stream);

/* networks/resnet_encoder.py:94  y = (x - mean) / std  elementwise (the encoder's input normalisation, 0.45 / 0.225).
 * The same arithmetic is available fused into the stem conv through fd_conv_desc.in_norm. */
int fd_input_normalize(const float* x, float* y, long n, float mean, float std, void* stream);
/* The pose networks' input in one pass (trainer.py:336-351 `torch.cat([inputs[("color_aug", f_i, 0)], inputs[("color_aug", f_j, 0)]], 1)`
 * for every source frame, stacked along the batch axis, followed by resnet_encoder.py:94): piece p copies `imgs` whole images
 * [imgs][C][H][W] from src[p] (device pointers, array on the HOST) to images dst_img[p] .. dst_img[p] + imgs - 1 of out
 * [n][Ct][H][W] at channel offset dst_ch[p], optionally as (x - mean) / std.  At most 16 pieces per call. */
int fd_stack_normalize(const float* const* src, const int* dst_img, const int* dst_ch, int n_pieces, int imgs, int C, int Ct, int H,
                       int W, float* out, int normalize, float mean, float std, void* stream);

/* out = a + b (feature fusion depth_decoder.py:70, pose_decoder.py:31) ; out = alpha*a + beta*b */
int fd_axpby(const float* a, const float* b, float* out, long n, float alpha, float beta, void* stream);

/* pose_decoder.py:44-46: out[n][c] = scale * mean over (H,W) of x[n][c]; and its adjoint. */
int fd_spatial_mean_fwd(const float* x, float* out, long planes, long plane_size, float scale, void* stream);
int fd_spatial_mean_bwd(const float* gout, float* gx, long planes, long plane_size, float scale, void* stream);

/* layers.py:284-302 compute_depth_errors on n matched (gt, pred) values: out[7] =
 * abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3.  ws: 7*256 floats. */
int fd_depth_errors(const float* gt, const float* pred, long n, float* out, float* ws, void* stream);

/* evaluate_depth.py:62-70 batch_post_process_disparity(l_disp, r_disp): l_disp / r_disp [planes][H][W] float32 (r_disp = the
 * prediction for the mirrored image, already flipped back) -> out [planes][H][W] float64, bit-exact vs the numpy expression. */
int fd_post_process_disparity(const float* l_disp, const float* r_disp, double* out, long planes, int H, int W, void* stream);

/* ------------------------------------------------------------------ optimiser ------------------ */

/* torch.optim.Adam step (trainer.py:129,247) over a flat parameter segment:
 *   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ; p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)
 * with step_size = lr/bc1, bc1 = 1-b1^t, bc2 = 1-b2^t computed by the caller.  grad_scale multiplies g first
 * (1/world_size averaging for data parallel).  */
int fd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                 float beta2, float eps, float bias_corr1, float bias_corr2, float grad_scale, void* stream);
/* Same update with the step counter and learning rate held on the device (state[0] = step count as float, incremented
 * by this call; state[1] = lr), so that a captured hipGraph of the training step stays valid across replays. */
int fd_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float* state, float beta1,
                     float beta2, float eps, float grad_scale, void* stream);
/* fd_adam_step_dev followed by optimizer.zero_grad(): the same update, bit for bit, and grad[0 .. n) is left all zeros by the
 * pass that read it (no separate fill of the gradient buffer). */
int fd_adam_step_dev_zero(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, float* state, float beta1,
                          float beta2, float eps, float grad_scale, void* stream);

/* Guarded Adam: a reduction over the flat gradient in front of the update, and an update that obeys the
 * decision the reduction left in device memory - no host read, no allocation, capturable.
 *
 * fd_grad_stats: x = grad[i] * grad_scale in float32 (the product Adam forms); per segment the sum of (double)x * (double)x in
 * float64, and the count of elements with !isfinite(x).  seg_offsets: n_seg + 1 ascending longs on the device, 0 first, n last
 * (1 <= n_seg <= FD_GUARD_MAX_SEGMENTS; a segment may be empty; entries outside 0 .. n are clamped, nothing outside grad is read).
 * Blocks write partial sums to ws (fd_grad_stats_ws_bytes(n, n_seg) bytes, 8-byte aligned), one block adds them through a fixed
 * tree: no atomics, a grid that depends on n alone, the same bits from two calls on any device.  Two launches.
 *   stats    (double): [0] norm = sqrt(sum of the segment sums, in segment order), [1] non-finite count, [2] coef, [3] skip (0 / 1),
 *                      [4 .. 4 + n_seg) the segments' norms
 *   counters (int64) : [0] steps skipped so far, [1] optimiser step of the first skip, [2] of the last skip (the caller starts
 *                      them at 0, -1, -1); the optimiser step is adam_state[0] + 1, the step this call would have been
 * skip = skip_nonfinite && count > 0.  coef = 1 if max_norm <= 0 or skip, else (double)(float)min(1, max_norm / (norm + 1e-6)):
 * torch.nn.utils.clip_grad_norm_'s factor, rounded to float32 once (a NaN norm that is not skipped gives 1).  n == 0 is legal. */
#define FD_GUARD_MAX_SEGMENTS 16
long fd_grad_stats_ws_bytes(long n, int n_seg);
int fd_grad_stats(const float* grad, long n, const long* seg_offsets, int n_seg, float grad_scale, float max_norm,
                  int skip_nonfinite, void* ws, double* stats, long* counters, const float* adam_state, void* stream);
/* The update behind that decision: state[0] advances only when stats[3] == 0; the gradient is (grad[i] * grad_scale) * (float)stats[2],
 * the rest is the update above statement for statement - with coef 1 and no skip the bits of param, both moments, grad and state are
 * those of the unguarded call with the same zero_grad.  A skipped step writes nothing to param or the moments; with zero_grad the
 * gradient is cleared in both cases, so that what was not finite does not reach the next window. */
int fd_adam_step_guarded(float* param, float* grad, float* exp_avg, float* exp_avg_sq, long n, float* state, float beta1,
                         float beta2, float eps, float grad_scale, const double* stats, int zero_grad, void* stream);

/* ------------------------------------------------------------------ sparse LiDAR --------------- */

/* gen2channel.py:60-117 get_4beam_2channel, gather formulation (race-free, bit-exact vs the
 * sequential reference): beam [B,1,H,W] -> out [B,2,H,W] (ch0 expanded depth, ch1 confidence).
 * Donor ROI rows [r0,r1), cols [c0,c1) (76,190,2,638 for 192x640); expand = 2. */
int fd_scatter_2channel(const float* beam, float* out, int B, int H, int W, int r0, int r1, int c0, int c1, int expand,
                        void* stream);

/* 3x3 stride-1 pad-1 convolution (nn.Conv2d / layers.Conv3x3 as above) through the 1-D Winograd F(2,3) transform: 1.5x fewer
 * MFMA cycles than the direct implicit GEMM.  Needs Cin % 16 == 0 and an even width (fd_conv3x3_wino_wt_floats returns 0
 * otherwise).  `wt` receives the transformed weights [4][Cout][3][Cin]; pass wt_ready = 1 to reuse them.  fd_conv2d_fwd routes
 * eligible convolutions here by itself; these entry points expose the path on its own (probes, tests). */
long fd_conv3x3_wino_wt_floats(const fd_conv_desc* d);
long fd_conv3x3_wino_ws_floats(const fd_conv_desc* d);
int fd_conv3x3_wino_fwd(const fd_conv_desc* d, const float* x, const float* w, const float* bias, float* y, float* wt, int wt_ready,
                        float* ws, void* stream);

/* LiDAR rasterisation (the step upstream of the scatter): kitti_utils.py:40-102 generate_depth_map + kitti_dataset.py:93-117
 * get_4beam + mono_dataset.py:193-198.  points [n][4] float32 (forward, left, up, reflectance), P_velo2im 3x4 float64 (device),
 * image im_h x im_w  ->  z-buffered sparse depth (float64; vel_depth != 0 stores the forward distance instead of the camera z,
 * kitti_utils.py:68-69), padded / cropped to target_h x target_w exactly as generate_depth_map(shape=[target_h, target_w]) does
 * (target_h <= 0: shape=None).  Outputs, either may be NULL:
 *   depth_out [padded_h][target_w] float64 = the function's return value  (padded_h = im_h + |target_h - im_h| - (2 if target_h < im_h))
 *   beam_out  [ceil(padded_h / 2)][ceil(target_w / 2)] float32 = 2x2 ceil-mode max-pool of it / 100 = the "4beam" network input.
 * Bit-exact vs the reference incl. its duplicate rule (oracle/rasterize.py).  ws: fd_velo_rasterize_ws_bytes bytes. */
long fd_velo_rasterize_ws_bytes(int n_points, int im_h, int im_w);
int fd_velo_rasterize(const float* points, int n_points, const double* P_velo2im, int im_h, int im_w, int vel_depth, int target_h,
                      int target_w, float* beam_out, double* depth_out, void* ws, void* stream);

/* evaluate_depth.py:349 `cv2.resize(pred_disp, (gt_width, gt_height))` on a float32 image (default INTER_LINEAR): OpenCV's
 * coefficient rule (source coordinate (float)((d + 0.5) * scale - 0.5) with the scale in double, floor, edges clamp with weight 0)
 * and its two float32 passes, horizontal first.  x [planes][Hin][Win] -> y [planes][Hout][Wout].  Restated from OpenCV's source
 * (resize.cpp); OpenCV is not available in the build image, so this entry point is parity-UNPINNED (oracle/evaluate.py). */
int fd_resize_linear_cv(const float* x, float* y, long planes, int Hin, int Win, int Hout, int Wout, void* stream);

/* ------------------------------------------------------------------ refiner inputs ------------- */

/* torch.median(x[mask] * scale) with mask = gate > 0 inside rows [y0,y1) x columns [x0,x1) of every [H][W] plane of the batch
 * (refiner.py:327-331: `torch.median(beam[mask] * 100.0)`): the LOWER median (rank (n-1)/2) over the whole batch, by radix select on
 * order-preserving integer keys - no sort, no host round trip for the selection size, result independent of the order in which
 * the selection was compacted.  out[0] = median (NaN when the selection is empty - the reference raises there - or holds a NaN),
 * out[1] = n.  x and gate: [B][H][W].  ws: fd_masked_median_ws_bytes(B, H, W) bytes. */
long fd_masked_median_ws_bytes(int B, int H, int W);
int fd_masked_median(const float* x, const float* gate, float scale, int B, int H, int W, int y0, int y1, int x0, int x1, float* out,
                     void* ws, void* stream);

/* refiner.py:316-348: the depth-map inputs of the refine decoder for ALL scales, written straight into the concatenated tensors
 * out[s] [B][1 + 3*catxy + 2][Hs][Ws] = (scaled_disp | Cat_xy(s-fold max-pooled depth, inv_K[s]) | s-fold max-pooled 2-channel map):
 * per scale, disp[s] (or, pool_disp0 != 0 = --refine_a0 true, the s-fold 2x2 ceil-mode max-pool of disp[0]) is up-sampled bilinearly
 * to H x W, turned into depth, scaled by median(beam[mask] * 100) / median(depth[mask]) (mask: beam > 0 inside the crop, medians over
 * the batch, fd_masked_median's rule), and scaled_disp = (bilinear down-sample of 1 / depth - 0.01) / 9.9.  Four launches, no
 * full-resolution intermediate.  Hs[s] * r == H, Ws[s] * r == W with r a power of two <= 8.  No gradient (the reference runs this
 * under no_grad / detaches the ratio; the decoder's inputs are leaves).  stats (may be NULL): [n_scales][4] = ratio,
 * median(depth[mask]), median(beam[mask] * 100), n.  ws: fd_refine_inputs_ws_bytes(cfg) bytes. */
typedef struct fd_refine_cfg {
    int B, H, W, n_scales;
    int Hs[4], Ws[4];
    int crop_y0, crop_y1, crop_x0, crop_x1;     /* refiner.py:329: rows 78..189, columns 23..616 */
    double min_depth, max_depth;
    int catxy, pool_disp0;
} fd_refine_cfg;
long fd_refine_inputs_ws_bytes(const fd_refine_cfg* cfg);
int fd_refine_inputs(const fd_refine_cfg* cfg, const float* const* disp, const float* beam, const float* two_cha,
                     const float* const* inv_K, float* const* out, float* stats, void* ws, void* stream);

/* ------------------------------------------------------------------ replay (round 6) ------------
 * Issue a recorded sequence of entry-point calls from ONE host call.  The Python layer pays 10 - 18 us of interpreter / ctypes /
 * autograd time per launch; the parts of a step that repeat the same calls on the same shapes and need no autograd graph - the
 * frozen stage-1 networks of refiner.py:299-330, validation forwards (trainer.py:390-423) - are recorded once and replayed here.
 *   fd_call_rec      one call: `fn` = index into the table of stream-ordered entry points (fd_replay_function_name / _signature:
 *                    every int-status entry point of this header whose last argument is the stream), `arg[i]` its arguments as
 *                    64-bit words (float / double arguments: the bits of a double), `kind[i]` & 15 = how arg[i] becomes the value:
 *                    0 literal, 1 arena + arg[i] bytes, 2 inputs[kind[i] >> 4] + arg[i] bytes, 3 the stream passed to fd_replay.
 *   fd_replay        runs the records in order on `stream`; stops at the first non-zero status and returns it.  Nothing is allocated
 *                    or synchronised: the caller owns `arena` (the records' intermediates and outputs live in it), the tensors
 *                    behind literal pointers (parameters, cached weight layouts, descriptors) and the inputs. */
#define FD_REPLAY_MAX_ARGS 24
typedef struct fd_call_rec {
    int fn, nargs;
    long long arg[FD_REPLAY_MAX_ARGS];
    unsigned short kind[FD_REPLAY_MAX_ARGS];
} fd_call_rec;
int fd_replay_function_count(void);
const char* fd_replay_function_name(int i);
const char* fd_replay_function_signature(int i);
int fd_replay(const fd_call_rec* recs, int n, void* arena, const void* const* inputs, int n_inputs, void* stream);

/* ------------------------------------------------------------------ graph-based depth correction --
 * gdc_old.py:74-250 GDC(pred_depth, gt_depth, calib, k, W_tol, recon_tol, consider_range, method='cg'): the stage-1 depth corrected
 * against sparse LiDAR (the Refiner's `inf_gdc` target, inf_gdc.py; evaluate_depth.py:387-405 --eval_gdc).  Five stream-ordered
 * calls; fusiondepth_amd/gdc.py drives them.  Unlike the rest of this header, the tensors here are float64 or int32 as stated per
 * argument (the reference computes in float64).  All arithmetic is float64; results are bit-reproducible run to run.
 *
 *   fd_gdc_prepare   gdc_old.py:66-71,108-109,121-167 (depth2ptc, filter_mask, filter_theta_mask, the masks): pred [H][W] float32,
 *                    gt [H][W] float64 (-1: no LiDAR), the rectified camera (c_u, c_v, f_u, f_v, b_x, b_y of
 *                    kitti_util_from_pse.py:97-102) and the pitch range in radians [pitch_lo, pitch_hi)  ->  pix [H*W] int32: the
 *                    pred_mask pixels (row-major), then the gt_mask pixels (row-major); counts [2] int32 = (N_PL, N_L).
 *                    ws: fd_gdc_prepare_ws_bytes(H, W) bytes.  The caller reads `counts` to size the solver workspace.
 *   fd_gdc_build     gdc_old.py:162-230 up to the solve: back-projected pred positions of the N = N_PL + N_L points, their exact
 *                    k + 1 nearest neighbours (float64 squared distances, ties by index, the point itself dropped), the
 *                    reconstruction weights in closed form (the (k+2)x(k+2) KKT system's solution does not depend on W_tol: it
 *                    cancels analytically, so W_tol is not an argument), b, A = [I - W_PLPL ; W_PLL] and its transpose, and the
 *                    start of scipy's cg on A^T A x = A^T b from x0 = x_info[:N_PL]: r = A^T b - A^T A x0, atol = recon_tol *
 *                    ||A^T b||.  Needs 1 <= k <= 16 and N >= k + 1.  ws: fd_gdc_ws_bytes(N_PL, N_L, k) bytes, starting with an
 *                    fd_gdc_state.  An exactly singular weight system (all k neighbours at one depth) sets state.fail.
 *   fd_gdc_cg_iters  n_iters iterations of scipy 1.15's cg loop (convergence test ||r|| < atol at the top of each iteration), four
 *                    launches each; once state.done is set every launch returns at once, so a caller enqueues iterations in
 *                    chunks and reads the state between them.  The caller bounds the total (maxiter).
 *   fd_gdc_finish    gdc_old.py:239-241: out [H][W] float32 = pred, the solution in the pred_mask pixels, gt wherever gt > 0; and
 *                    state.rnorm = ||r||.  ws == NULL and pix == NULL: out = pred (the failure path - the reference's caller
 *                    keeps the input depth when GDC raises). */
typedef struct fd_gdc_state {
    double rho, rho_prev;         /* r.r of the current / previous iteration */
    double atol, bnorm, rnorm;    /* recon_tol * ||A^T b||, ||A^T b||, ||r|| (rnorm: written by fd_gdc_finish) */
    int iterations;               /* completed CG iterations */
    int done, converged, fail, zero_rhs;   /* done: converged, failed, or ||A^T b|| == 0 (the solution is then A^T b = 0) */
} fd_gdc_state;
long fd_gdc_prepare_ws_bytes(int H, int W);
int fd_gdc_prepare(const float* pred, const double* gt, int H, int W, double c_u, double c_v, double f_u, double f_v, double b_x,
                   double b_y, double pitch_lo, double pitch_hi, int* pix, int* counts, void* ws, void* stream);
long fd_gdc_ws_bytes(int N_PL, int N_L, int k);
int fd_gdc_build(const float* pred, const double* gt, const int* pix, int N_PL, int N_L, int k, int H, int W, double c_u, double c_v,
                 double f_u, double f_v, double b_x, double b_y, double recon_tol, void* ws, void* stream);
int fd_gdc_cg_iters(void* ws, int N_PL, int N_L, int k, int n_iters, void* stream);
int fd_gdc_finish(const float* pred, const double* gt, const int* pix, int N_PL, int N_L, int k, int H, int W, void* ws, float* out,
                  void* stream);

/* ------------------------------------------------------------------ training images (uint8) ---- */

/* The image half of a training item, datasets/mono_dataset.py:85-104: `Resize(..., ANTIALIAS)`, `ColorJitter` and `ToTensor` on
 * PIL images.  uint8 images are [H][W][3] (what a decoder produces), outputs for the networks are float32 [3][H][W] planes.
 * Pinned bit for bit to PIL 12 (tests/augment_ref.py restates the rules; torchvision's PIL branch is a thin mapping onto them).
 *
 * fd_resize_lanczos_u8: Pillow's 8-bit antialiased Lanczos resample, src [N][Hin][Win][3] -> dst [N][Hout][Wout][3]: a horizontal
 *   pass into ws (uint8), then a vertical pass.  xtab / ytab (device, int32): per output column / row the record
 *   (first tap, tap count, k coefficients), k = kx / ky = 2 * ceil(3 * max(in, out) / out) + 1; coefficient = int(w * 2^22 +- 0.5) of
 *   the float64 weight, built by the caller on the host (data_ops.lanczos_table).  pixel = clip((2^21 + sum) >> 22).
 *   mirror (device, int32 [N], may be NULL): frames with a non-zero entry are read flipped left-right (kitti_dataset.py:59-60 flips
 *   before resizing).  src and ws 16-byte aligned; ws: fd_resize_lanczos_u8_ws_bytes bytes.
 * fd_color_jitter_u8: n_images images described by a device table, one launch sequence for all of them whatever their sizes.
 *   Image i is read at src + src_off, has order[0 .. n_ops) of the operations 0 brightness, 1 contrast, 2 saturation, 3 hue applied
 *   with factor[op] (every intermediate is uint8, as between PIL calls; n_ops = 0 copies), and is written as uint8 to
 *   dst_u8 + u8_off and / or as v / 255 planes to dst_planes + planes_off + c * H * W (an offset < 0: not written); plain_off
 *   receives the planes of the image as read, so one pass over a level writes `color` and `color_aug`.  An operation may appear
 *   at most once in order (an entry that repeats one is skipped).  Contrast
 *   blends towards int(mean(L) + 0.5) of the image as it stands at that point: an exact integer sum, reduced by wave shuffle, LDS
 *   and a fixed-order final pass.  An image whose extent leaves src_bytes / dst_bytes / planes_floats is skipped as a whole.
 *   max_pixels: the largest H * W of the table (sizes the grid).  ws: fd_color_jitter_u8_ws_bytes(n_images) bytes, 8-byte
 *   aligned; after the call int32 mean[n_images] (-1: no contrast) stands at byte fd_color_jitter_u8_means_offset(n_images) of it.
 * fd_u8_to_planes: ToTensor.  src [N][H][W][3] -> dst + n * dst_image_stride + c * H * W, float32(v) / 255 correctly rounded. */
typedef struct fd_jitter_desc {
    long src_off;                 /* bytes */
    long u8_off;                  /* bytes, < 0: no uint8 output */
    long planes_off;              /* floats, < 0: no plane output of the jittered image */
    long plain_off;               /* floats, < 0: none; planes of the image BEFORE the operations (`color` beside `color_aug`) */
    int H, W;
    float factor[4];              /* brightness, contrast, saturation as float32 (PIL casts them to C float itself); [3] unused */
    int order[4];                 /* operation ids in application order, each at most once */
    int n_ops;                    /* 0 .. 4 */
    int hue_shift;                /* uint8 added to H: trunc(h * 255) mod 256 of the DOUBLE h, computed by the caller */
} fd_jitter_desc;
long fd_resize_lanczos_u8_ws_bytes(int N, int Hin, int Win, int Hout, int Wout);
int fd_resize_lanczos_u8(const uint8_t* src, uint8_t* dst, int N, int Hin, int Win, int Hout, int Wout, const int* xtab, int kx,
                         const int* ytab, int ky, const int* mirror, void* ws, void* stream);
long fd_color_jitter_u8_ws_bytes(int n_images);
long fd_color_jitter_u8_means_offset(int n_images);
int fd_color_jitter_u8(const uint8_t* src, long src_bytes, uint8_t* dst_u8, long dst_bytes, float* dst_planes, long planes_floats,
                       const fd_jitter_desc* desc, int n_images, long max_pixels, void* ws, void* stream);
int fd_u8_to_planes(const uint8_t* src, float* dst, int N, int H, int W, long dst_image_stride, void* stream);

/* ------------------------------------------------------------------ raw Velodyne scans -> sparse LiDAR ----
 * sparsify/sparsify.py:32-136 (gen_sparse_points + pto_ang_map), batched: S scans in one call, a constant number of launches
 * whatever S is.  A scan is [n][4] float32 (x, y, z, intensity); the scans are concatenated in `points` and `offsets` (device,
 * int32 [S + 1], offsets[0] = 0, offsets[S] = total_points) says where each starts.
 *   filter   x_lo <= x < x_hi, y_lo <= y < y_hi, z_lo <= z < z_hi (the reference: [0,120) x [-50,50) x [-2.5,1.5)).
 *   cell     d = sqrt(x*x + y*y + z*z), r = sqrt(x*x + y*y) in float32, summed left to right, no fused multiply-add; an exact 0
 *            becomes float32(1e-6); asin(y / r) and asin(z / d) as float32; from there float64, as numpy 2 promotes the
 *            reference's expression: column = int((radians(45) - asin(y/r)) / radians(90 / W)), row = int((radians(2) -
 *            asin(z/d)) / radians(0.4 * 64 / H)), truncated towards zero and clamped to [0, W-1] / [0, H-1].  asin is the one
 *            step numpy does not round correctly; here it is evaluated in double on the float32 quotient and rounded once.
 *   winner   the LAST point of a cell in scan order (the reference's fancy-index assignment) = the highest index: an integer
 *            atomic max, order independent.
 *   output   the winners of the occupied cells of rows[0 .. n_rows) (in the order given; no row twice), columns ascending, as
 *            their original 16 bytes: slab [S][cap][4] float32 with cap = n_rows * W, kept points first, the remainder filled
 *            with (-1, 0, 0, 0) - generate_depth_map drops x < 0 first, so a padded slab rasterises like the compacted scan -
 *            and counts (device, int32 [S]).  Nothing is read back.
 *   random_sample = N > 0 (sparsify.py:15-29,81-87): of those points, keep the ones with a non-zero float64 norm of (x,y,z,i)
 *            and u < N * 1.8 / n_keep, one u per compacted point in output order, n_keep = the number with a non-zero norm.
 *            u comes from `uniforms` (device, float64 [S][cap]: reproduces np.random.uniform draws injected by the caller) or,
 *            when that is NULL, from the library's counter-based generator keyed by (seed, keys[s], output slot): a scan's
 *            selection depends on nothing else.  keys: device, uint64 [S], needed only then.
 *   cells    optional (device, int32 [total_points]): row * W + column of every point that passed the filter, -1 otherwise.
 *   ws: fd_sparsify_ws_bytes(cfg) bytes, 16-byte aligned.  Run-to-run identical: integer atomics and fixed-order sums only. */
#define FD_SPARSIFY_MAX_ROWS 64
typedef struct fd_sparsify_cfg {
    int S;                        /* scans */
    int H, W;                     /* angular grid: 1 <= H <= 1024 rows, W columns */
    int n_rows;                   /* 1 .. FD_SPARSIFY_MAX_ROWS */
    int rows[FD_SPARSIFY_MAX_ROWS];
    float x_lo, x_hi, y_lo, y_hi, z_lo, z_hi;
    int random_sample;            /* N; 0: off */
    int reserved;
    unsigned long long seed;      /* the library's own generator (uniforms == NULL) */
} fd_sparsify_cfg;
long fd_sparsify_ws_bytes(const fd_sparsify_cfg* cfg);
int fd_sparsify_scans(const float* points, const int* offsets, long total_points, const fd_sparsify_cfg* cfg,
                      const double* uniforms, const unsigned long long* keys, float* slab, int* counts, int* cells, void* ws,
                      void* stream);

/* fd_velo_rasterize for S scans in one call (four launches whatever S is).  Scan s is points[offsets[s] .. offsets[s + 1]) when
 * `offsets` (device, int32 [S + 1]) is given, else points[s * n_max .. (s + 1) * n_max) - a padded slab of fd_sparsify_scans;
 * n_max bounds every scan's length.  desc (device, [S]): the scan's P_velo2im, image size and flip flag; max_im_h / max_im_w
 * bound the image sizes (they size ws).  target_h / target_w and vel_depth are common.  Every scan must pad to the same
 * padded_h rows (im_h + |target_h - im_h|, minus 2 when target_h < im_h) and have im_w <= target_w: one that does not, or that
 * leaves max_im_h / max_im_w, gets an all-zero output.  beam_out [S][(padded_h + 1) / 2][(target_w + 1) / 2] float32 and / or
 * depth_out [S][padded_h][target_w] float64, each scan bit-identical to fd_velo_rasterize on it, mirrored left-right where
 * desc[s].flip is set.  ws: fd_velo_rasterize_batch_ws_bytes(S, max_im_h, max_im_w) bytes. */
typedef struct fd_raster_desc {
    double P[12];                 /* P_velo2im, row-major 3x4 */
    int im_h, im_w;
    int flip, reserved;
} fd_raster_desc;
long fd_velo_rasterize_batch_ws_bytes(int S, int max_im_h, int max_im_w);
int fd_velo_rasterize_batch(const float* points, const int* offsets, int n_max, int S, const fd_raster_desc* desc, int max_im_h,
                            int max_im_w, int vel_depth, int target_h, int target_w, int padded_h, float* beam_out,
                            double* depth_out, void* ws, void* stream);

/* ------------------------------------------------------------------ batched bilinear resize ("inf_gdc" key) ----
 * kitti_dataset.py:163-171: F.interpolate(map, [h, w], mode="bilinear", align_corners=False), then fliplr where the item is
 * flipped - for B planes of different sizes in ONE launch.  packed (device, float32 [packed_floats]) holds the planes; desc
 * (device, [B]) says where plane b starts (in floats), its size, and whether its result is mirrored.  out [B][out_h][out_w].
 * Arithmetic = ATen's CPU kernel in float32, bit for bit, per axis:
 *   scale = (float)n_in / (float)n_out;  src = fmaf(scale, (float)d + 0.5f, -0.5f) (one rounding), clamped below at 0;
 *   i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - (float)i0, l0 = 1.0f - l1
 * and the blend, width first, the second product of each line rounded on its own:
 *   top = fmaf(hx, x[y0][x0], lx * x[y0][x1]);  bot = fmaf(hx, x[y1][x0], lx * x[y1][x1]);  out = fmaf(hy, top, ly * bot).
 * The mirror acts on the resized plane, out[b][y][x] = resized[b][y][out_w - 1 - x]: resizing the mirrored source rounds
 * differently.  (torch's CPU path for outputs of about 32x64 and below rounds differently again; not covered.)
 * A descriptor that does not lie inside the packed buffer yields a NaN plane; nothing outside the buffer is read. */
typedef struct fd_resize_desc {
    long offset;                  /* first float of the plane in `packed` */
    int h_in, w_in;
    int mirror, reserved;
} fd_resize_desc;
int fd_resize_bilinear_batch(const float* packed, long packed_floats, const fd_resize_desc* desc, int B, int out_h, int out_w,
                             float* out, void* stream);

/* ------------------------------------------------------------------ KITTI depth completion ----
 * Depth keys (datasets/kitti_completion.py:51-80 get_depth, completion_dataset.py:314-367): S 16-bit depth PNGs of different sizes,
 * decoded into one packed uint16 buffer, become [S][channels][ceil(canvas_h / pool)][ceil(canvas_w / pool)] float32 in ONE launch.
 * Per plane the descriptor names a window of the canvas and the source pixel (in left-right mirrored coordinates where `mirror`
 * is set: mirrored column x is source column w - 1 - x) that lands on the window's first pixel; canvas pixels outside the window
 * are 0.  bottom_crop is a window that covers the canvas with (src_y, src_x) = (h - 352, j); the zero pad is (src_y, src_x) =
 * (0, 0) with the window at (384 - h, (1280 - w) / 2); crop-then-pad is both.  Each output is
 *   max over its pool x pool block, clipped at the canvas edge (ceil_mode), of ((float)v / div0), then / div1
 * - two correctly rounded float32 divisions in that order, no reciprocal - written `channels` times.  A descriptor whose plane
 * does not lie inside `packed`, whose window leaves the canvas or whose source rectangle leaves the plane yields a NaN plane;
 * nothing outside the buffer is read.  packed and desc 8-byte aligned, out 16-byte aligned. */
typedef struct fd_depth_png_desc {
    long offset;                  /* first uint16 of the plane in `packed` */
    int h, w;                     /* the decoded PNG */
    int mirror;                   /* fliplr before crop / pad */
    int src_y, src_x;             /* source pixel (after mirroring) of canvas pixel (win_y, win_x) */
    int win_y, win_x, win_h, win_w;   /* the filled window of the canvas */
    int reserved;
} fd_depth_png_desc;
int fd_depth_png_keys(const uint16_t* packed, long packed_elems, const fd_depth_png_desc* desc, int S, int canvas_h, int canvas_w,
                      int pool /*1|2*/, int channels /*1|2*/, float div0, float div1, float* out, void* stream);

/* Scoring (evaluate_completion.py:31-48 compute_errors, :297-355), per image n of pred / gt [N][H][W], mask m = gt > gt_min.
 * Two entry points because --eval_gdc corrects the scaled prediction between them.
 * fd_completion_medians: out[n] = { ratio, median(gt[m]), median((pred * pred_scale)[m]), count }, the medians numpy's (for an
 *   even count the float32 mean of the two middle order statistics: (a + b) rounded to float32, then halved - not torch's lower
 *   median), ratio = median(gt) / median(pred) in float32; NaN for all three when nothing is selected or a selected prediction is
 *   NaN.  Radix select over keys formed from the planes in every pass: no list, no sort.  The ws argument is IGNORED by this entry point
 *   (pass NULL); it is there so that the two calls take the same arguments.
 * fd_completion_errors: p = pred * pred_scale (* ratio[n] when ratio != NULL), p < lo -> lo, p > hi -> hi, then in float32 as numpy
 *   evaluates it: gt * 1000 - p * 1000, its square and abs; 1 / (gt * 0.001) - 1 / (p * 0.001), its square and abs.  The four sums
 *   over m run in float64 (a fixed grid of partial sums, added in index order: bitwise reproducible, no float atomics);
 *   out[n] = { sqrt(mean sq) = rmse [mm], mae [mm], irmse [1/km], imae [1/km], count } as float64, NaN where the count is 0.
 *   ws: fd_completion_ws_bytes(N, H, W) bytes, 8-byte aligned. */
long fd_completion_ws_bytes(int N, int H, int W);
int fd_completion_medians(const float* pred, const float* gt, int N, int H, int W, float gt_min, float pred_scale,
                          float* out /*[N][4]*/, void* ws, void* stream);
int fd_completion_errors(const float* pred, const float* gt, const float* ratio /*[N] or NULL*/, int N, int H, int W,
                         float gt_min, float pred_scale, float lo, float hi, double* out /*[N][5]*/, void* ws, void* stream);

/* ------------------------------------------------------------------ Eigen-split scoring --------
 * The per-image loop of evaluate_depth.py:344-478 (without GDC) for N images whose ground-truth maps differ in size, in ONE call of
 * 6 launches (5 without median scaling), whatever N is (csrc/eigen_eval.hip).
 *   disp     [M][h][w] predicted disparities;  packed: the ground-truth planes, image n at `offset`, H x W, row-major.
 *   desc     DEVICE array of N descriptors.  The mask of image n is  gt > gt_lo && gt < gt_hi  inside rows [y0, y1), columns [x0, x1)
 *            (gt_hi = +inf: no upper bound).  A descriptor whose plane leaves `packed`, whose window leaves the plane or whose `pred`
 *            is not in [0, M) gives a NaN row with count -1; nothing outside the buffers is read.
 * At every selected pixel, and only there: OpenCV's float32 INTER_LINEAR resize of disp[pred] to H x W from its four taps (the
 * arithmetic of fd_resize_linear_cv: horizontal pass first, separate multiplies and adds), 1 / that (IEEE division), * pred_scale.
 * The (gt, pred) pairs are compacted in row-major order (counts per window row, a scan, then the writes: every position is a function
 * of the data alone).  median_scaling != 0: ratio = median(gt) / median(pred) with numpy's medians (radix select over the compact
 * lists; an even count takes the float32 mean of the two middle values) and pred *= ratio.  Then p = pred < lo ? lo : pred > hi ? hi : pred
 * (a NaN stays) and the terms of compute_errors (evaluate_depth.py:42-60) in float32, one rounding per numpy operation; the log term
 * is (float)(log((double)gt) - log((double)p)) squared in float32 (numpy's float32 log is not correctly rounded and cannot be
 * restated bit for bit).  The sums run in float64 over a fixed grid of partials, added in index order: no float atomics, bitwise
 * reproducible.
 *   out[n] = { abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, count } as float64; ratio is NaN without median scaling; an
 *   empty selection gives NaN metrics and count 0, a NaN prediction what numpy gives (NaN for the first four and the ratio, a1-a3 = 0).
 *   ws: fd_eigen_scores_ws_bytes(N, max_rows, list_cap) bytes, 8-byte aligned, where max_rows >= y1 - y0 of every image and
 *   list_cap >= the sum of (y1 - y0) * (x1 - x0) over the images.  N <= 4096.  packed, desc 8-byte aligned. */
typedef struct fd_eigen_desc {
    long offset;                  /* first float of the ground-truth plane in `packed` */
    int H, W;                     /* its size */
    int pred;                     /* index of the disparity plane */
    int y0, y1, x0, x1;           /* the mask window: rows [y0, y1), columns [x0, x1) */
    int reserved;
} fd_eigen_desc;
long fd_eigen_scores_ws_bytes(int N, int max_rows, long list_cap);
int fd_eigen_scores(const float* disp, int M, int h, int w, const float* packed, long packed_floats, const fd_eigen_desc* desc, int N,
                    int max_rows, long list_cap, float gt_lo, float gt_hi, float pred_scale, int median_scaling, float lo, float hi,
                    double* out /*[N][9]*/, void* ws, void* stream);

/* ------------------------------------------------------------------ per-class Eigen-split scoring
 * evaluate_depth.py's --per_semantic loop (:451-467): for every class c, compute_errors on the selected pixels whose label is c
 * (csrc/eigen_class.hip).
 * fd_eigen_class_scores: fd_eigen_scores' arguments from disp through hi, unchanged in meaning, and its launches; then
 *   labels   packed_floats BYTES: the uint8 label plane of image n is H x W, row-major, and starts at BYTE desc[n].offset (the planes
 *            lie back to back like the ground truth's, so they start at arbitrary - odd included - addresses; they are read by bytes).
 *   K        1 .. 256 classes; a pixel whose label is >= K belongs to no class.
 *   out      [N][9], exactly fd_eigen_scores' out for the same inputs, bit for bit.
 *   class_out[n][c] = { abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, count } as float64 over the selected pixels of image n whose
 *            label is c: the SAME ratio (the whole image's), clamps and float32 terms as out[n], float64 sums.  While the pairs are
 *            compacted, each selected pixel's label goes to a uint8 list at the pair's index; then one workgroup of 256 threads per
 *            (class, image) walks the image's compact list: thread t adds pairs t, t + 256, ... of its class in index order, the
 *            lanes of a wave add through a fixed shuffle tree, the four waves are added in wave order.  No partials, no float
 *            atomics: bitwise reproducible.  A class without pixels gives eight zeros (the reference's np.zeros(7), count 0); a NaN
 *            prediction in a class gives NaN for the first four and 0 for a1-a3, as in out; a refused descriptor (count -1 in out)
 *            gives zero rows.
 *   ws: fd_eigen_class_scores_ws_bytes(N, max_rows, list_cap, K) bytes, 8-byte aligned (fd_eigen_scores' layout followed by the label
 *   list).  K outside 1 .. 256 or sizes outside fd_eigen_scores' limits: status -1, fd_last_error set, nothing launched (the size
 *   query returns 0).  packed, desc, out, class_out 8-byte aligned.
 * fd_class_errors: the class kernel alone on n >= 0 matched pairs that are already scaled: p = pred < lo ? lo : pred > hi ? hi : pred,
 *   then as above -> class_out[c], c < K.  The same workgroup shape, thread stride and tree: the same pairs in the same order give
 *   the same bits by either entry point.  One launch. */
long fd_eigen_class_scores_ws_bytes(int N, int max_rows, long list_cap, int K);
int fd_eigen_class_scores(const float* disp, int M, int h, int w, const float* packed, long packed_floats, const fd_eigen_desc* desc,
                          int N, int max_rows, long list_cap, float gt_lo, float gt_hi, float pred_scale, int median_scaling, float lo,
                          float hi, const unsigned char* labels, int K, double* out /*[N][9]*/, double* class_out /*[N][K][8]*/,
                          void* ws, void* stream);
int fd_class_errors(const float* gt, const float* pred, const unsigned char* labels, long n, int K, float lo, float hi,
                    double* class_out /*[K][8]*/, void* stream);

/* ------------------------------------------------------------------ training-time scoring ------
 * compute_depth_losses (trainer.py:598-630) + compute_depth_errors (layers.py:284-302) per image, for N images whose ground-truth maps
 * differ in size, in ONE call of 6 launches, whatever N is (csrc/val_scores.hip; the kernels are fd_eigen_scores' under another
 * compile-time rule, csrc/score_lists.h).  The arguments are fd_eigen_scores':
 *   depth    [M][h][w] predicted DEPTHS (outputs[("depth", 0, 0)]);  packed, desc, N, max_rows, list_cap, ws as above.
 *            The mask of image n is  gt > 0  inside rows [y0, y1), columns [x0, x1) (the caller passes the Garg crop 153:371, 44:1197
 *            clipped to the plane, as slicing clips it).  A descriptor whose plane leaves `packed`, whose window leaves the plane or
 *            whose `pred` is not in [0, M) gives a NaN row with count -1; nothing outside the buffers is read.
 * At every selected pixel, and only there: ATen's CPU bilinear rule with align_corners=False resamples depth[pred] to H x W - the
 * arithmetic of fd_resize_bilinear_batch: scale = (float)n_in / (float)n_out, src = fmaf(scale, d + 0.5f, -0.5f) clamped at 0, the
 * blend width first, top = fmaf(hx, a, lx * b), out = fmaf(hy, top, ly * bot) - then p = p < lo ? lo : p > hi ? hi : p (a NaN stays).
 * The (gt, p) pairs are compacted in row-major order.  The medians are torch's: the LOWER order statistic, rank (n - 1) / 2, NaN
 * when the list holds one.  ratio = median(gt) / median(p) (IEEE float32 division), p = p * ratio, the clamp again, then the terms of
 * compute_depth_errors in float32, one rounding per operation (IEEE divisions for gt / p and p / gt; 1.25, 1.5625 and 1.953125 are
 * exact); the log term is (float)(log((double)gt) - log((double)p)) squared in float32, as in fd_eigen_scores and for its reason.
 * The sums run in float64 over a fixed grid of partials, added in index order: no float atomics, bitwise reproducible.
 *   out[n] = { abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, count } as float64; an empty selection gives NaN metrics and
 *   count 0, a NaN prediction what torch gives (NaN for the first four and the ratio, a1-a3 = 0).
 *   ws: fd_val_scores_ws_bytes(N, max_rows, list_cap) bytes, 8-byte aligned.  N <= 4096.  packed, desc, out 8-byte aligned. */
long fd_val_scores_ws_bytes(int N, int max_rows, long list_cap);
int fd_val_scores(const float* depth, int M, int h, int w, const float* packed, long packed_floats, const fd_eigen_desc* desc, int N,
                  int max_rows, long list_cap, float lo, float hi, double* out /*[N][9]*/, void* ws, void* stream);

/* ------------------------------------------------------------------ the Completor's training-time scoring
 * compute_depth_losses (completor.py:728-762) + compute_depth_errors (layers.py:284-302) per image, in ONE call of 6 launches, whatever
 * N is (csrc/completion_val.hip; fd_val_scores' kernels under a third compile-time rule, csrc/score_lists.h).  The arguments are
 * fd_val_scores' plus gt_min; what differs from its rule:
 *   the mask of image n is  gt > gt_min  inside rows [y0, y1), columns [x0, x1): a float32 comparison against a float32 (the caller
 *   passes (float)0.1, as torch compares a float32 tensor with the Python scalar 0.1).  The caller passes the whole plane as the
 *   window, or with --completion_eigen_crop 153:371, 44:1197 clipped to the plane as slicing clips it.
 *   after  p = clamp(p * ratio, lo, hi)  both sides are scaled to millimetres, g' = g * 1000.0f and p' = p * 1000.0f, one float32
 *   rounding each, and the seven terms of compute_depth_errors are formed on g' and p' as fd_val_scores forms them on g and p.
 * Everything else is fd_val_scores': ATen's CPU bilinear rule on depth[pred] at the selected pixels only (equal sizes included: the
 * rule is then the identity), the clamp before torch's LOWER medians, ratio = median(gt) / median(p) on the UNSCALED lists, float64 sums
 * over the fixed grid of partials added in index order (no float atomics, bitwise reproducible), the bad-descriptor row (NaN, count -1).
 *   out[n] = { abs_rel, sq_rel, rmse [mm], rmse_log, a1, a2, a3, ratio, count } as float64.
 *   ws: fd_completion_val_scores_ws_bytes(N, max_rows, list_cap) bytes, 8-byte aligned.  N <= 4096.  packed, desc, out 8-byte aligned. */
long fd_completion_val_scores_ws_bytes(int N, int max_rows, long list_cap);
int fd_completion_val_scores(const float* depth, int M, int h, int w, const float* packed, long packed_floats, const fd_eigen_desc* desc,
                             int N, int max_rows, long list_cap, float gt_min, float lo, float hi, double* out /*[N][9]*/, void* ws,
                             void* stream);

/* ------------------------------------------------------------------ detection depth export -----
 * The dense part of export_detection.py:317-392 for N maps of different sizes in ONE launch (csrc/detection.hip): the whole predicted
 * depth map at each image's own size, scaled and quantised to the 16-bit PNG payload.
 *   disp     [M][h][w] predicted disparities.
 *   desc     DEVICE array of N descriptors: map n is H x W, row-major, at element `offset` of the packed outputs, computed from
 *            disp[pred].  Planes lie back to back at arbitrary (odd included) element offsets; nothing is assumed about alignment.
 *            A descriptor whose plane leaves [0, packed_elems), whose size is not positive or whose `pred` is not in [0, M) writes
 *            nothing.  max_H / max_W >= every H / W (they size the grid; a larger map is written only up to them).
 * For every output pixel, each step ONE float32 rounding, no contraction:
 *   d = OpenCV's float32 INTER_LINEAR resize of disp[pred] to H x W (the arithmetic of fd_resize_linear_cv / fd_eigen_scores:
 *       coefficients in double -> float, horizontal pass first, separate multiplies and adds);
 *   p = 1 / d (IEEE division);  p *= pred_scale;  p *= ratio[n] when ratio != NULL;  q = p * 256.
 * depth_out (float32, packed_elems, or NULL) receives p, u16_out (uint16, packed_elems, or NULL) the quantised q; at least one of
 * them is given.  The quantiser is truncation toward zero - numpy's astype(np.uint16) in range.  Out of range numpy's cast is
 * undefined; here it is DEFINED: NaN and negative q -> 0, q >= 65535 (+inf included) -> 65535.
 * No workspace, no atomics; every store is a plain vector store, 16 bytes per lane wherever the row segment is 16-byte aligned
 * (the address decides, not the descriptor), narrower at a row's head and tail.  N <= 65535.
 * fd_depth_quantize_u16: the same quantiser on a contiguous float64 plane of n values (the map GDC returns); q = x * 256 is a float64
 * product there, as numpy computes it for the reference's float64 map. */
typedef struct fd_export_desc {
    long offset;                  /* first element of the map in the packed outputs */
    int H, W;                     /* its size */
    int pred;                     /* index of the disparity plane */
    int reserved;
} fd_export_desc;
int fd_depth_export(const float* disp, int M, int h, int w, const fd_export_desc* desc, int N, long packed_elems, int max_H, int max_W,
                    float pred_scale, const float* ratio /*[N] or NULL*/, float* depth_out, uint16_t* u16_out, void* stream);
int fd_depth_quantize_u16(const double* x, uint16_t* out, long n, void* stream);

/* ------------------------------------------------------------------ pseudo-LiDAR point clouds --
 * Pseudo-LiDAR's project_depth_to_points for N dense depth maps of different sizes, packed back to back as fd_depth_export writes
 * them, in THREE launches whatever N is and without atomics of any kind (csrc/pseudo_lidar.hip): every pixel back-projected into the
 * Velodyne frame, filtered, and the kept points written as float32 (X, Y, Z, 1) records - the KITTI .bin layout.
 *   depth    packed float32 planes; desc: DEVICE array of N fd_export_desc - map n is H x W, row-major, at element `offset`; `pred` is
 *            ignored.  A descriptor whose plane leaves [0, packed_elems), whose size is not positive or whose H / W exceeds max_H /
 *            max_W is skipped: it contributes no point, starts[n + 1] == starts[n].  max_H / max_W size the grid and the workspace.
 *   calib    DEVICE array of N fd_points_calib (144 bytes each): the camera of kitti_util_from_pse.py's Calibration and the rectified
 *            camera -> Velodyne map A = R^T inv(R_rect_00), t = -(R^T T) of calib_velo_to_cam.txt.
 * For pixel column u, row v (integers) and z = (double)depth[v][u], every step in float64, each operation rounded ONCE, no contraction,
 * IEEE divisions, in exactly this order:
 *   x = ((u - c_u) * z) / f_u + b_x
 *   y = ((v - c_v) * z) / f_v + b_y
 *   X = ((A[0] * x + A[1] * y) + A[2] * z) + t[0]        Y, Z likewise with A[3..5], t[1] and A[6..8], t[2]
 *   keep = (X >= 0) && (Z < max_high)                     a NaN falls out through the comparisons; there is no other filter
 *   point = (float)X, (float)Y, (float)Z, 1.0f
 * A kept point has a finite-or-infinite X and Z by the predicate; its Y can be a NaN only for an infinite depth (inf - inf), and the sign
 * and payload of that NaN are the hardware's - the one thing the rule leaves open.
 * Kept points follow in row-major pixel order (numpy's boolean indexing), the maps back to back in descriptor order.
 *   points   float32, 16-byte aligned, room for 4 * packed_elems floats; each kept point is ONE 16-byte store at points + 4 * index.
 *            Only the first 4 * starts[N] floats are written.  (Overlapping descriptors can name more pixels than packed_elems; a
 *            point whose index is >= packed_elems is counted in `starts` but not written.)
 *   starts   long [N + 1]: the index of the first point of each map, the total last.
 *   ws       fd_points_export_ws_bytes(N, max_H) bytes, 16-byte aligned (0: sizes out of range): two ints per row - its count and
 *            its first slot, in separate arrays, because the scan's workgroups read the counts of each other's maps.
 * N is 1 .. 65535, max_H * max_W < 2^30.  The position of a point depends on the predicate alone, never on arrival: two calls give
 * the same bytes.  The scan reads the row counts of all earlier maps once per map - quadratic in N, meant for chunks of tens of maps. */
typedef struct fd_points_calib {
    double c_u, c_v, f_u, f_v, b_x, b_y; /* Calibration of camera 2 */
    double A[9];                         /* row-major 3 x 3 */
    double t[3];
} fd_points_calib;
long fd_points_export_ws_bytes(int N, int max_H);
int fd_points_export(const float* depth, const fd_export_desc* desc, const fd_points_calib* calib, int N, long packed_elems, int max_H,
                     int max_W, double max_high, void* ws, float* points, long* starts /*[N + 1]*/, void* stream);

/* ------------------------------------------------------------------ evaluate_depth --visualize --
 * The two pictures of evaluate_depth.py:407-449 for N <= 64 maps of different sizes, packed back to back as fd_depth_export and
 * fd_eigen_scores pack them, in at most 9 launches and one memset whatever N is (csrc/visualize.hip).
 *   The map: EITHER disp [M][h][w] with pred_scale and ratio ([N] or NULL) - the depth is then formed exactly as fd_depth_export forms
 *            it (OpenCV's float32 INTER_LINEAR rule through csrc/cv_resize.h, 1 / ., * pred_scale, * ratio[n]) - OR depth_in, packed_floats
 *            dense float32 values at the descriptors' offsets (the map GDC returns, rounded to float32 once).  Exactly one is given.
 *   packed_gt / desc  the packed ground truth and the DEVICE descriptors of fd_eigen_scores; gt_lo / gt_hi its bounds (gt_hi = +inf: no
 *            upper bound).  packed_gt may be NULL when err is.  With depth_in, `pred` is not read.  A descriptor whose plane leaves
 *            [0, packed_floats), whose window leaves the plane or whose `pred` is not in [0, M) writes nothing; nothing outside the
 *            buffers is read.  max_pixels >= H * W of every image (it sizes the grids).
 *   lut_disp / lut_err  two colour tables of 256 x 3 uint8, RGB order.
 * Outputs, each optional (NULL skips its work), at least one given:
 *   depth_out  float32, packed_floats: the depth maps.
 *   stats      [N][2] float32 (vmin, vmax) of d' = 1.0f / depth (IEEE): vmin = min d'; vmax = np.percentile(d', 95) as numpy 2 computes
 *            it for float32 input, in float32 throughout: q = 95.0f / 100.0f, pos = (float)(n - 1) * q, k = floor(pos), g = pos - k,
 *            a = sorted[k], b = sorted[min(k + 1, n - 1)], vmax = a + (b - a) * g, or b - (b - a) * (1.0f - g) where g >= 0.5f, or a
 *            where a == b.  The two order statistics come from a radix select over the whole plane (up to 64 workgroups per image, LDS
 *            histograms merged into one per image and pass with integer atomics, one launch per 8-bit pass; a fifth pass counts the
 *            keys <= a's and takes the smallest key above and the minimum).
 *   color    uint8, 3 * packed_floats: image n is [H][W][3] at byte 3 * offset.  xn = (float)((double)(d' - vmin) / ((double)vmax -
 *            (double)vmin)) - a float32 difference, a float64 quotient rounded to float32 once -, 0 where vmin == vmax; xa = xn * 256.0f; index = trunc(xa) clamped to 0 .. 255 (xa >= 256 -> 255; NaN and
 *            negative -> 0; a non-finite d' -> 0); the pixel is lut_disp[index] - matplotlib's Normalize and colormap call.
 *   err      uint8, 3 * err_pixels: the pictures [ceil(H/2)][ceil(W/2)][3] back to back in descriptor order (a refused descriptor takes no room).  At a pixel inside the
 *            window whose ground truth is selected (gt > gt_lo && gt < gt_hi): v = trunc(80.0f - clamp(|depth - gt|, 0, 2) * 40.0f)
 *            and the colour lut_err[v]; elsewhere 0.  Then the 2 x 2 maximum per channel (rows and columns beyond an odd edge count
 *            as 0) and (220, 220, 220) where all three channels are 0.  A picture that would leave err_pixels is not written.
 * Each float32 step is one rounding, no contraction, no float atomics: two calls give the same bits.  The pictures are written as
 * 16-byte stores wherever the address allows, byte by byte before the first and after the last 16-byte boundary of an image.
 *   ws: fd_vis_render_ws_bytes(N, packed_floats) bytes, 16-byte aligned (0: sizes out of range). */
long fd_vis_render_ws_bytes(int N, long packed_floats);
int fd_vis_render(const float* disp, int M, int h, int w, float pred_scale, const float* ratio /*[N] or NULL*/, const float* depth_in,
                  const float* packed_gt, long packed_floats, const fd_eigen_desc* desc, int N, long max_pixels, float gt_lo, float gt_hi,
                  const unsigned char* lut_disp, const unsigned char* lut_err, unsigned char* color, unsigned char* err, long err_pixels,
                  float* stats /*[N][2]*/, float* depth_out, void* ws, void* stream);

/* ------------------------------------------------------------------ train --log_images --
 * The image summaries of trainer.py:656-681 for J <= 64 items of a batch: one uint8 RGB contact sheet [Hs][Ws][3] per item, J sheets
 * back to back, in two launches and one memset whatever J, the number of scales and the number of frames are (csrc/log_images.hip).
 *   A sheet is a stack of row blocks (one per scale); a row block holds tiles side by side, each with its top edge on the block's.
 *   Every byte of every sheet is written by the call: a pixel in no tile is 0.  The tile table holds J * NT entries, item-major; the
 *   geometry (kind, y, x, h, w, aux, slot) of tile i is the same for every item, the pointers are the item's own.
 *   kind 0 colour      p0 = float [3][h][w]                                   -> q(r), q(g), q(b)
 *   kind 1 prediction  p0 = the source frame's colours [3][h][w], p1 = the disparity [h][w] of scale 0, p2 = K, p3 = inv_K, p4 = T
 *                      (float [4][4] each): depth = 1 / (lo + span * disp), X = depth * inv_K[:3,:3] (x, y, 1), pix = P X / ((P X)_z + eps)
 *                      with P = (K T)[:3], then F.grid_sample(bilinear, border, align_corners=False) of the colours - the steps and the
 *                      conventions of fd_photo_fwd_ex, restated.  h, w >= 2.
 *   kind 2 disparity   p0 = float [h][w]: utils.normalize_image - ma, mi the plane's float32 maximum and minimum,
 *                      d = (float)((double)ma - (double)mi), 1e5 where ma == mi, the pixel q((x - mi) / d) with an IEEE division; a NaN
 *                      anywhere in the plane makes every pixel 0 (torch's max() is NaN then).  slot = the tile's rank among the item's
 *                      disparity tiles; cfg.disp_tile[slot] = its index.
 *   kind 3 automask    p0 = uint8 [h][w], the argmin index fd_photo_*_fwd leaves in `sel`: 255 where index > aux - 1, else 0.
 *   kind 4 mask        p0 = float [h][w] -> q(x).
 *   Single-channel kinds fill the three channels alike.  q(x) = trunc(min(max(x * 255.0f, 0), 255)), NaN -> 0, in float32.
 *   ws: fd_log_sheets_ws_bytes(J, n_disp) bytes, 16-byte aligned (0: out of range).  After the call it holds, per item and disparity
 *   tile, four uint32: key(ma), ~key(mi), 1 if a NaN was seen, 0 - key(v) = bits ^ 0xffffffff for a negative v, bits | 0x80000000 else.
 *   tiles_host: the same table in host memory; its geometry is checked against cfg before anything is launched. */
typedef struct fd_log_tile {
    const void* p0; const void* p1; const void* p2; const void* p3; const void* p4;
    int kind, y, x, h, w;            /* the tile's place in the sheet */
    int aux;                         /* kind 3: the number of identity losses */
    int slot;                        /* kind 2: rank among the item's disparity tiles */
    int reserved;
} fd_log_tile;
typedef struct fd_log_cfg {
    int Hs, Ws;                      /* the sheet */
    int n_rows, n_disp;              /* row blocks (<= 8), disparity tiles per item (<= 8) */
    int row_y[8], row_h[8];          /* a row block's top edge and height; the blocks follow each other down the sheet */
    int row_first[8], row_count[8];  /* its tiles, left to right: row_first[0] = 0, row_first[r + 1] = row_first[r] + row_count[r] */
    int disp_tile[8];                /* the index of the item's k-th disparity tile */
    float lo, span;                  /* (float)(1 / max_depth), (float)(1 / min_depth - 1 / max_depth): disp_to_depth */
    float eps;                       /* Project3D's 1e-7 */
    int reserved;
} fd_log_cfg;
long fd_log_sheets_ws_bytes(int J, int n_disp);
int fd_log_sheets(const fd_log_tile* tiles_host, const fd_log_tile* tiles_dev, int J, int NT, const fd_log_cfg* cfg, unsigned char* sheets,
                  void* ws, void* stream);

/* ------------------------------------------------------------------ baseline JPEG frames --
 * Pillow's `Image.open(f).convert("RGB")` of a baseline JPEG, split where GPU loaders split it: the serial Huffman decoding on the
 * host (csrc/jpeg_entropy.h: plain C++, no GPU call, no globals, thread-safe, usable on a machine without a GPU), everything after it
 * on the device (csrc/jpeg.hip).  libjpeg's default back half is integer arithmetic throughout, so the result is held to Pillow's
 * bytes (tests/jpeg_ref.py restates the rules below in numpy, entropy decoder included).
 *
 * Covered streams: SOF0, and SOF1 at 8 bits; Huffman coding; ONE interleaved scan; three-component YCbCr (a JFIF marker, or no Adobe
 * marker and component ids other than 'R','G','B') with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, or one-component greyscale;
 * restart intervals; custom Huffman tables; 8- or 16-bit quantisation tables.  NOT covered: progressive, lossless, arithmetic coding,
 * 12 bits, CMYK / Adobe RGB, 4:4:0 and every other sampling, multi-scan baseline, DNL.  For those `covered` is 0, the probe still
 * returns 0 once it has read the frame header, and the decoder returns FD_JPEG_UNCOVERED: a status, never a guess.
 *
 * Neither host function reads outside [file, file + n) or writes outside coef[0 .. coef_cap) and qt[0 .. 192), whatever the bytes are.
 * A status other than 0 leaves its reason in fd_last_error() (thread-local): FD_JPEG_TRUNCATED when the data ends before the last
 * block (or inside the headers), FD_JPEG_CORRUPT for an undefined Huffman code, a coefficient index above 63, a missing or wrong
 * restart marker, a bad segment.
 *   coef  the QUANTISED coefficients, int16 [blocks][64] in natural (row-major, de-zigzagged) order, component after component, each
 *         component's blocks row-major over its PADDED block grid blocks_h[c] x blocks_w[c] (whole MCUs: blocks_w[0] = mcus_x * h_samp,
 *         blocks_w[1] = blocks_w[2] = mcus_x; a greyscale frame has ceil(W / 8) x ceil(H / 8) blocks).  coef_cap counts int16 values;
 *         info->coef_count of them are written (blocks past an end-of-block are zero).  The DC predictor wraps in int16.
 *   qt    uint16 [3][64], natural order: the table of each component (greyscale: three copies). */
#define FD_JPEG_OK 0
#define FD_JPEG_BAD_ARGS 1
#define FD_JPEG_NOT_JPEG 2
#define FD_JPEG_UNCOVERED 3
#define FD_JPEG_TRUNCATED 4
#define FD_JPEG_CORRUPT 5
#define FD_JPEG_CAPACITY 6
typedef struct fd_jpeg_info {
    int width, height;
    int components;                  /* as the frame header says: 1, 3 (or 2, 4: not covered) */
    int h_samp, v_samp;              /* luma sampling factors (1, 1 for greyscale); 0 when not covered */
    int covered;
    int blocks_w[3], blocks_h[3];    /* the padded block grid of each component */
    int restart_interval;
    int reserved;
    long coef_count;                 /* int16 values the frame needs: 64 * the sum of blocks_w[c] * blocks_h[c] */
} fd_jpeg_info;
int fd_jpeg_probe(const unsigned char* file, long n, fd_jpeg_info* info);
int fd_jpeg_entropy_decode(const unsigned char* file, long n, int16_t* coef, long coef_cap, uint16_t* qt /*[3][64]*/, fd_jpeg_info* info);

/* The device half: one chunk of 1 <= N <= 65535 frames of different sizes and samplings in TWO launches whatever N is,
 * no atomics, no workspace beyond the component planes the descriptors place inside `staging`.
 *   staging   the device copy of the chunk's staging buffer, 16-byte aligned, staging_bytes long; every offset below is in bytes from it.
 *   desc      DEVICE array of N fd_jpeg_desc, 8-byte aligned (it may lie inside staging).
 *   out       uint8; frame n is written as [height][width][3] RGB at out + out_off.  16-byte stores at the address's 16-byte
 *             boundaries, single bytes before the first and after the last boundary of a frame.
 * kind 0 (coefficients): coef_off -> the int16 coefficients as fd_jpeg_entropy_decode writes them (16-byte aligned), qt_off -> its
 *   uint16 [3][64] tables (16-byte aligned), plane_off -> room for the uint8 component planes, 8 * blocks_h[c] rows of 8 * blocks_w[c]
 *   bytes, component after component (16-byte aligned; the planes need not be uploaded, and no other region may overlap them).
 * kind 1 (raw): coef_off -> height * width * 3 bytes of RGB that a host decoder wrote; launch B copies them.
 * A descriptor whose frame leaves `out`, whose width or height is outside 1 .. 65535 or whose 3 * width * height exceeds 2^31 - 1 is skipped.  A descriptor that is otherwise
 * unusable - a region that leaves staging, a misaligned offset, an unknown kind, sampling or component count - yields a ZERO frame.  Nothing outside
 * the two buffers is read or written.  Two calls on the same input give the same bytes.
 *
 * Launch A, per 8 x 8 block (jidctint.c, ISLOW; CONST_BITS = 13, PASS1_BITS = 2), all in int32 with wrap-around:
 *   d[k] = coef[k] * qt[k]                                     a 32-bit product
 *   the 1-D transform of eight values x0 .. x7 with the multipliers FIX(0.298631336) = 2446, FIX(0.390180644) = 3196, FIX(0.541196100) =
 *   4433, FIX(0.765366865) = 6270, FIX(0.899976223) = 7373, FIX(1.175875602) = 9633, FIX(1.501321110) = 12299, FIX(1.847759065) = 15137,
 *   FIX(1.961570560) = 16069, FIX(2.053119869) = 16819, FIX(2.562915447) = 20995, FIX(3.072711026) = 25172:
 *     z1 = (x2 + x6) * 4433; t2 = z1 - x6 * 15137; t3 = z1 + x2 * 6270; t0 = (x0 + x4) << 13; t1 = (x0 - x4) << 13
 *     t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
 *     o0 = x7, o1 = x5, o2 = x3, o3 = x1; z1 = o0 + o3; z2 = o1 + o2; z3 = o0 + o2; z4 = o1 + o3; z5 = (z3 + z4) * 9633
 *     o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
 *     o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4
 *     y0, y7 = t10 +- o3; y1, y6 = t11 +- o2; y2, y5 = t12 +- o1; y3, y4 = t13 +- o0
 *   first down every column with y -> (y + (1 << 10)) >> 11, then along every row with y -> (y + (1 << 17)) >> 18 (arithmetic shifts;
 *   libjpeg's all-zero shortcuts give the same values), then the sample = limit(y & 1023) with limit(i) = 128 + i for i < 128, 255 for
 *   i < 512, 0 for i < 896, i - 896 above: the level shift and libjpeg's masked range-limit table in one.
 * Launch B, per pixel (jdsample.c, jdcolor.c), dw = ceil(width / 2) and dh = ceil(height / 2) the chroma plane's REAL size:
 *   1x1 and greyscale: the chroma sample is the pixel's own.
 *   2x1 (h2v1 fancy): c = x >> 1, a = C[y][c]; even x: a at c = 0, else (3 a + C[y][c - 1] + 1) >> 2; odd x: a at c = dw - 1, else
 *       (3 a + C[y][c + 1] + 2) >> 2.
 *   2x2 (h2v2 fancy): r = y >> 1, far = r - 1 for an even y, r + 1 for an odd one, clamped to [0, dh - 1] (the real rows, not the padded
 *       block rows); s(c) = 3 C[r][c] + C[far][c]; even x: (4 s(c) + 8) >> 4 at c = 0, else (3 s(c) + s(c - 1) + 8) >> 4; odd x:
 *       (4 s(c) + 7) >> 4 at c = dw - 1, else (3 s(c) + s(c + 1) + 7) >> 4.
 *   dw <= 2: plain replication, C[y >> (v_samp - 1)][x >> 1], as jinit_upsampler chooses.
 *   R = clamp(Y + ((91881 * (Cr - 128) + 32768) >> 16)); B = clamp(Y + ((116130 * (Cb - 128) + 32768) >> 16));
 *   G = clamp(Y + ((-22554 * (Cb - 128) + 32768 - 46802 * (Cr - 128)) >> 16)); arithmetic shifts, clamp to 0 .. 255.
 *   Greyscale writes Y to the three channels.
 * Bit-exactness: the result equals Pillow's (libjpeg-turbo's) decode for every stream whose dequantised coefficients d[k] fit int16 -
 * every 8-bit encoder's output does.  Outside that range libjpeg's own paths disagree with each other; the result then follows the
 * int32 rule above and is not pinned to Pillow. */
typedef struct fd_jpeg_desc {
    long coef_off;                   /* kind 0: the coefficients; kind 1: the RGB bytes */
    long qt_off;
    long plane_off;
    long out_off;                    /* into `out` */
    int kind;                        /* 0 coefficients, 1 raw RGB */
    int width, height;
    int components;                  /* 1 or 3 */
    int h_samp, v_samp;              /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for greyscale) */
    int reserved[2];
} fd_jpeg_desc;
int fd_jpeg_reconstruct(void* staging, long staging_bytes, const fd_jpeg_desc* desc, int N, unsigned char* out, long out_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------ PNG frames --
 * Pillow's `Image.open(f).convert("RGB")` of an 8-bit PNG and `np.asarray(Image.open(f))` of a 16-bit grey one, split like the JPEG
 * decoder above: the serial half - the chunk walk and the inflate of the IDAT stream - on the host (csrc/png_inflate.h: plain C++, no
 * zlib, no GPU call, no globals, no allocation, thread-safe, usable on a machine without a GPU), the scanline filters on the device
 * (csrc/png.hip).  Every step is integer arithmetic on bytes, so the result is held to Pillow's bytes (tests/png_ref.py restates the
 * chunk walk and the filters in numpy; zlib.decompress restates the inflate).
 *
 * Covered files: non-interlaced; colour type 2 at bit depth 8 (RGB, bpp 3), colour type 0 at bit depth 8 (grey, bpp 1) and colour type
 * 0 at bit depth 16 (depth maps, bpp 2), none of them with a tRNS chunk.  NOT covered: palette, alpha (colour types 4 and 6), tRNS,
 * Adam7, bit depths 1 / 2 / 4, 16-bit RGB, animated PNG (an acTL chunk), more than 2^31 - 1 scanline bytes.  For those `covered` is 0,
 * the probe still returns 0 once it has read IHDR, and fd_png_inflate returns FD_PNG_UNCOVERED: a status, never a guess.
 *
 * fd_png_inflate treats the payloads of the consecutive IDAT chunks as ONE zlib stream - a payload may end at any byte, inside a code
 * or inside a stored block's LEN, and may be empty - and writes exactly raw_bytes = height * (1 + row_bytes) FILTERED bytes to dst:
 * per scanline its filter-type byte, then row_bytes = width * bpp bytes.  Stored, fixed and dynamic blocks; `dst` is its own window.
 * Neither function reads outside [file, file + n) or writes outside dst[0 .. dst_cap), whatever the bytes are.  A status other than 0
 * leaves its reason in fd_last_error() (thread-local).  What is checked, and the status of a miss:
 *   FD_PNG_NOT_PNG     the 8-byte signature.
 *   FD_PNG_CORRUPT     IHDR: first chunk, 13 bytes, its CRC-32, non-zero size, compression and filter method 0, a colour type and bit
 *                      depth that go together.  zlib header: CM = 8, CINFO <= 7, FCHECK, no FDICT.  Deflate: block type 3; LEN against
 *                      NLEN; more than 286 literal/length or 30 distance codes; a code-length repeat with nothing before it or past the
 *                      last code; no end-of-block code; an over-subscribed code, or an incomplete one other than at most one code of
 *                      length 1 (zlib's rule: the one-code distance tree is a code, an incomplete code-length code is not); a symbol
 *                      no code stands for (an unused pattern, lengths 286 / 287, distances 30 / 31); a distance beyond the bytes written;
 *                      MORE than raw_bytes of output.  After the stream: its Adler-32 against the bytes written; a filter-type byte
 *                      above 4; an IEND chunk that is not the twelve bytes it has to be (its CRC with them).
 *   FD_PNG_TRUNCATED   a file that ends inside a chunk header, an IDAT payload or its CRC field, inside the stream, or before a whole
 *                      IEND; a stream that ends with FEWER than raw_bytes of output.  Only the whole file returns 0.
 *   FD_PNG_CAPACITY    dst_cap < raw_bytes (nothing is written).
 * CRCs: IHDR's and IEND's are verified.  The IDAT chunks' are NOT - Pillow does not verify them either; the stream's Adler-32, which
 * is verified, covers the same bytes - and neither are those of the ancillary chunks, which are skipped unread.  Bytes behind the end
 * of the zlib stream inside the IDAT run are ignored, as zlib ignores them. */
#define FD_PNG_OK 0
#define FD_PNG_BAD_ARGS 1
#define FD_PNG_NOT_PNG 2
#define FD_PNG_UNCOVERED 3
#define FD_PNG_TRUNCATED 4
#define FD_PNG_CORRUPT 5
#define FD_PNG_CAPACITY 6
typedef struct fd_png_info {
    int width, height;
    int bit_depth, colour_type, interlace;    /* as IHDR says */
    int covered;
    int bpp;                         /* bytes per pixel: 3, 1 or 2; 0 when not covered */
    int reserved;
    long row_bytes;                  /* width * bpp; 0 when not covered */
    long raw_bytes;                  /* height * (1 + row_bytes); 0 when not covered */
    long reserved2[2];
} fd_png_info;
int fd_png_probe(const unsigned char* file, long n, fd_png_info* info);
int fd_png_inflate(const unsigned char* file, long n, unsigned char* dst, long dst_cap, fd_png_info* info);

/* The device half: one chunk of 1 <= N <= 65535 frames of different sizes and formats in TWO launches whatever N and the sizes are, no
 * atomics, no workspace.
 *   staging   the device copy of the chunk's staging buffer, 16-byte aligned, staging_bytes long; every raw_off is in bytes from it.
 *             Its first N * sizeof(fd_png_desc) bytes hold a copy of `desc`: the caller uploads table and scanlines as ONE buffer.
 *   desc      HOST array of the N descriptors.  Every one is checked here before anything is launched; the first bad one refuses the
 *             whole call with a non-zero status and its index and reason in fd_last_error().  The kernels read the copy inside staging and
 *             apply the same check again, skipping what fails it, so a copy that differs from `desc` cannot take them outside the
 *             two buffers.
 *   out       16-byte aligned; frame n is written at out + out_off: mode 0 (rgb) uint8 [height][width][3], a grey sample written to
 *             all three channels as convert("RGB") does; mode 1 (gray16) host-order uint16 [height][width], the big-endian sample
 *             swapped on the store (out_off even).  16-byte stores at the address's 16-byte boundaries, single bytes before the first
 *             and after the last boundary of a frame.
 * kind 0 (scanlines): raw_off -> the height * (1 + width * bpp) filtered bytes as fd_png_inflate writes them; (bpp, mode) is (3, rgb),
 *   (1, rgb) or (2, gray16).  kind 1 (raw): raw_off -> the frame's bytes exactly as they go to `out` (a host decoder wrote them; bpp
 *   is ignored); launch B copies them.
 * The check: kind 0 or 1, mode 0 or 1, a (bpp, mode) pair from the list; width and height in 1 .. 65535 with at most 2^31 - 1 output
 *   and scanline bytes; raw_off at or behind the table, and the frame's source, rounded up to a multiple of 16 bytes for kind 0 (the
 *   kernel loads aligned 16-byte pieces), inside staging_bytes; out_off >= 0 and the frame inside out_bytes.  Regions of different
 *   descriptors must not overlap; this is not checked, and an overlap cannot take the kernels outside the two buffers.
 * Launch A (k_png_unfilter) reconstructs the scanlines IN PLACE, one workgroup per frame.  With a = the byte bpp to the left, b = the
 *   byte above, c = the byte above-left (each 0 outside the picture), mod 256: None adds nothing, Sub a, Up b, Average (a + b) >> 1 on
 *   the 9-bit sum, Paeth the one of a, b, c nearest to p = a + b - c, ties in the order a, b, c.  FD_PNG_BAND_ROWS lanes walk as many
 *   rows as a skewed wavefront: lane r is one pixel behind lane r - 1 and takes b (and, a step later, c) from it through LDS; a frame
 *   taller than that goes band after band in the same workgroup, the lane before a band's first row re-reading the reconstructed row
 *   above it as an unfiltered one.  Width + rows - 1 steps per band.  Each lane streams its row through registers in aligned 16-byte
 *   loads issued three pieces ahead, and writes whole aligned words except at the row's two ends.  Every reconstructed row's filter
 *   byte is set to 0 (None): STAGING IS OVERWRITTEN, and a second call on the same two buffers gives the same bytes.
 * Launch B (k_png_store) writes `out` in 16-byte pieces from the reconstructed rows (or the raw bytes of kind 1).
 *
 * Measured on one MI355X, twice (profiles/png_decode_time.log; 36 frames of 1242x375 written by Pillow with default settings from
 * textured synthetic content, 1122 KB per file, rows filtered Sub and Up only): a batch through data_ops.decode_png_batch 15.12 /
 * 14.92 ms against 38.46 / 37.13 ms for Pillow on 16 threads + np.stack + upload; KITTIRAWBatches from the PNG tree 836.6 / 784.0
 * against 319.4 / 281.4 items/s (the larger run-to-run spread 264.4 / 121.3), the trainer fed by it 414.2 / 416.2 against 254.0 /
 * 250.0 images/s.  One host thread, per frame: fd_png_inflate 2.84 / 2.86 ms, zlib.decompress (1.2.11) of the same stream 3.57 /
 * 3.58 ms, Pillow's whole decode 4.51 / 4.57 ms - the inflate beats zlib's by 1.25x.  Host phase 12.0 / 12.5 ms, upload 50.3 MB in
 * 1.0 / 0.9 ms, the two launches 1.68 ms = 105x their traffic bound (100.6 MB at 6.3 TB/s) and 11 % of the batch: the compiler waits
 * for each lane's row load where it is issued, so a wavefront step costs a memory latency (open).  NOT
 * measured: a real KITTI tree (another encoder: other filter choices and compression), more than one rank sharing the host's 16
 * threads, the completion loader end to end. */
#define FD_PNG_BAND_ROWS 512
typedef struct fd_png_desc {
    long raw_off;                    /* kind 0: the filtered scanlines; kind 1: the finished bytes */
    long out_off;                    /* into `out` */
    int kind;                        /* 0 scanlines, 1 raw */
    int width, height;
    int bpp;                         /* kind 0: 3 (RGB), 1 (grey), 2 (16-bit grey) */
    int mode;                        /* 0 rgb, 1 gray16 */
    int reserved[3];
} fd_png_desc;
int fd_png_band_rows(void);
int fd_png_unfilter(void* staging, long staging_bytes, const fd_png_desc* desc, int N, unsigned char* out, long out_bytes, void* stream);

/* ------------------------------------------------------------------------------ PNG outputs --
 * The encoder: PNG files that decode to the input value for value in Pillow, zlib and fd_png_inflate + fd_png_unfilter above.  It is
 * split the other way round than the decoder: filtering has no serial dependency, and a deflate stream of literals and distance-1
 * runs only (zlib's Z_RLE strategy) needs no match search, so pixels in, file bytes out is all device work; the host builds the
 * Huffman codes from per-block histograms in between (csrc/png_deflate.h: plain C++, no zlib, no GPU call, usable without a GPU) and
 * fills the three CRC-32 fields at the end.  tests/png_enc_ref.py restates the whole stream in numpy; the files are held to its bytes.
 *
 * Covered inputs: uint8 [H][W][3] (colour type 2, bpp 3), uint8 [H][W] (colour type 0 at depth 8, bpp 1), host-order uint16 [H][W]
 * (colour type 0 at depth 16, samples big-endian in the file, bpp 2); 1 <= W, H <= 65535, at most 2^31 - 1 scanline bytes a frame;
 * frames of different sizes and kinds in one batch of 1 <= N <= 65535.  No interlacing, palette, alpha or ancillary chunks.
 *
 * THE STREAM.  R = W * bpp, P = 1 + R.
 *   Filter.   Each row chooses among None, Sub, Up, Average, Paeth (types 0 .. 4) with the decoder's arithmetic: a = the byte bpp to
 *             the left, b = the byte above, c = above-left, each 0 outside the frame; Average (a + b) >> 1 on the 9-bit sum; Paeth the
 *             one of a, b, c nearest to a + b - c, ties in the order a, b, c.  Cost = the sum over the row's R bytes of |int8(byte)|;
 *             the smallest cost wins, a tie goes to the lowest type.
 *   Tokens.   Each scanline (its filter byte first) is cut into maximal runs of equal bytes; runs never cross a scanline.  A run of
 *             length L is, in order: one literal; (L - 1) / 258 matches of length 258; the remainder m = (L - 1) % 258 as one match if
 *             m >= 3, else as m literals.  Every match has distance 1.
 *   Blocks.   FD_PNG_ENC_BLOCK_ROWS scanlines are one deflate block, BTYPE 2, BFINAL on the frame's last.  Literal/length lengths are
 *             Huffman lengths of the block's counts plus one end-of-block, at most 15 bits; the code-length code at most 7 bits.  Tree
 *             rule: merge the two nodes of smallest (weight, id) until one is left - a leaf's id is its symbol, the k-th merged node's
 *             is 286 (or 19) + k.  Limit rule: while the deepest leaf is deeper than the limit, every weight w becomes (w + 1) >> 1
 *             and the tree is built again.  Canonical codes.  The distance tree: one code of length 1 (HDIST field 0) when the block
 *             has a match, one zero length when it has none.  HLIT is trimmed to the last used symbol, at least 257; HCLEN to the
 *             last used entry of the permuted order, at least 4; a code-length code with one used symbol gets a second code of length
 *             1 (symbol 0, or 1 if 0 is the used one).  The HLIT + 1 lengths are run-length coded greedily: at a position with value
 *             v and r equal values from there on - v == 0: r >= 11 -> symbol 18 for min(r, 138); else r >= 3 -> symbol 17 for r; else
 *             a 0; v != 0: v once, then symbol 16 for min(r, 6) while r >= 3 remain, then the rest one by one.
 *   Wrapping. Signature; IHDR; ONE IDAT holding 78 01, the blocks, zero bits up to the byte, the Adler-32 of the H * P filtered
 *             bytes; IEND.  A file takes 57 + 2 + ceil(stream bits / 8) + 4 bytes, known after the plan and before any is written.
 *
 * THE CALLS, in order, for one batch:
 *   fd_png_enc_layout  host.  In: src, width, height, bpp of every descriptor.  Out: their ws_off / first_row / first_block /
 *                      first_group, and *sizes.  The caller allocates `work` (sizes.work_bytes, 16-byte aligned).
 *   fd_png_enc_filter  copies the table to work[0 ..), clears the statistics, LAUNCH A (k_png_enc_filter): a workgroup of four waves
 *                      takes FD_PNG_ENC_GROUP_ROWS = 4 scanlines of one frame, a wave per scanline, a lane per byte, 64 bytes a step.
 *                      A first walk over the row sums the five costs; a second writes the chosen filter's bytes to the workspace
 *                      (16-bit samples byte-swapped on the load), counts the row's tokens into LDS (a run is closed by the lane at
 *                      the next run's first byte, found from the wave's ballot of "differs from the byte before"), and sums the
 *                      Adler pair (sum d_j, sum (P - j) d_j) mod 65521.  At the end one global integer add per non-zero LDS count.
 *   (download)         work[stat_off .. stat_off + stat_bytes): uint32 [blocks][FD_PNG_ENC_HIST] - 286 literal/length counts without
 *                      end-of-block, [286] the matches, [287] unused - then uint32 [rows][2] Adler pairs.
 *   fd_png_enc_plan    host.  Fills blocks[0 .. sizes.blocks) - lengths, reversed codes, header bits, exact size in bits = header +
 *                      sum count[s] * (len[s] + extra[s]) + matches, first bit inside the frame's stream - and per descriptor adler,
 *                      stream_bits, out_off, out_bytes (the files one behind the other from byte 0); *total_bytes = their sum.
 *   fd_png_enc_emit    `blocks` is HOST memory (pinned for an asynchronous copy); it and the table are checked (every block inside
 *                      its file) and copied to work; `out` (out_bytes >= total_bytes rounded up to a multiple of 4, plus 4; 4-byte
 *                      aligned) is cleared.  LAUNCH B (k_png_enc_rowbits): a wave per scanline sums its tokens' bits.  LAUNCH C
 *                      (k_png_enc_emit): a wave per scanline; its first bit = the block's + the header's + the bits of the block's
 *                      earlier rows (at most 63 values, one wave reduction); per 64-byte step an exclusive wave scan of the closed
 *                      runs' bits places each run, whose lane ORs its tokens in.  The wave of a block's first row also ORs the
 *                      header in, that of its last row the end-of-block, that of the frame's first row the signature, IHDR, chunk
 *                      lengths and types, 78 01 and the Adler-32.  Every write is an integer atomic OR on a 32-bit word of the
 *                      cleared buffer, bounds-checked against the frame's file, so writers may share words and two calls give the
 *                      same bytes.  No float atomics anywhere.
 *   (download)         out[0 .. total_bytes) into pinned memory.
 *   fd_png_enc_finish  host, per file: the CRC-32s of IHDR, IDAT and IEND, in place (eight bytes a step).
 * THREE launches per batch (A, B, C) whatever N, the sizes and the block counts are, plus two clears and three small uploads: the
 * descriptor table before A, and again with the plan's fields before B, both from the caller's pageable table (staged copies); the
 * block table before B.
 *
 * Measured on one MI355X, twice, routes alternating (profiles/png_encode_time.log; textured synthetic content): 64 maps of 375x1242
 * uint16 through data_ops.encode_png_batch 14.24 / 14.17 ms against 277.7 / 276.3 ms for Pillow on 16 threads after the download; one
 * 768x4480 RGB sheet 3.37 / 3.26 against 327.1 / 326.6 ms; files +6 % (maps) and -0.1 % (sheets) against Pillow's.  The three launches:
 * 1.253 ms for the 64 maps = 25x their traffic bound (DESIGN.md section 25 says why, and what is left open).  export_detection on a
 * synthetic tree of 32 maps: 262.2 / 261.4 ms with pil, 126.1 / 126.2 ms with device - recommended there; the Trainer with log_images
 * at the default log frequency: 115.83 / 115.72 against 115.82 / 115.96 steps/s - a tie inside the spread, not recommended there.
 * NOT measured: a real KITTI tree (real depth maps
 * and frames compress differently from synthetic content), real detector-side readers of the files, file-system write time. */
#define FD_PNG_ENC_BLOCK_ROWS 64
#define FD_PNG_ENC_GROUP_ROWS 4
#define FD_PNG_ENC_HIST 288
#define FD_PNG_ENC_HEADER_WORDS 128
typedef struct fd_png_enc_desc {
    const void* src;                 /* DEVICE pixels, contiguous; 2-byte aligned for bpp 2 */
    long ws_off;                     /* layout: the frame's filtered scanlines inside work */
    long out_off, out_bytes;         /* plan: the file inside out */
    long stream_bits;                /* plan: the deflate blocks' bits */
    int width, height;
    int bpp;                         /* 3 (RGB), 1 (grey), 2 (16-bit grey) */
    int first_row, first_block, first_group;   /* layout: the batch-wide index of the frame's first scanline / block / row group */
    unsigned adler;                  /* plan */
    int reserved[3];
} fd_png_enc_desc;
typedef struct fd_png_enc_sizes {
    long rows, blocks, groups;       /* of the whole batch */
    long raw_bytes;                  /* sum of H * P */
    long stat_off, stat_bytes;       /* the download */
    long rowbits_off, table_off, ws_off;
    long work_bytes;
} fd_png_enc_sizes;
typedef struct fd_png_enc_block {
    unsigned long long bit_off;      /* the block's first bit inside its frame's deflate stream */
    unsigned long long bits;         /* header + tokens + end-of-block */
    unsigned header_bits;
    unsigned dist_len;               /* 1: the block has matches, each followed by the one-bit distance code 0 */
    unsigned header[FD_PNG_ENC_HEADER_WORDS];   /* the header's bits, LSB first */
    unsigned short code[288];        /* canonical, bit-reversed */
    unsigned char len[288];
    unsigned reserved[2];
} fd_png_enc_block;
int fd_png_enc_block_rows(void);
int fd_png_enc_layout(fd_png_enc_desc* desc, int N, fd_png_enc_sizes* sizes);
int fd_png_enc_filter(void* work, long work_bytes, const fd_png_enc_desc* desc, int N, void* stream);
int fd_png_enc_plan(fd_png_enc_desc* desc, int N, const unsigned* stats, fd_png_enc_block* blocks, long* total_bytes);
int fd_png_enc_emit(void* work, long work_bytes, const fd_png_enc_desc* desc, int N, const fd_png_enc_block* blocks,
                    unsigned char* out, long out_bytes, void* stream);
int fd_png_enc_finish(unsigned char* files, long nbytes, const fd_png_enc_desc* desc);

/* ------------------------------------------------------------------------------ JPEG outputs --
 * The encoder: uint8 [H][W][3] pixels in, the bytes Pillow (libjpeg's defaults: baseline, standard tables, optimize off, no restart
 * markers, no smoothing) writes for Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=s) out.  Everything from the pixels to
 * the stuffed entropy-coded bytes and FF D9 is device work; the host lays out the batch, builds the tables and writes the 623 header
 * bytes in front of each stream (csrc/jpeg_enc_host.h: plain C++, no GPU call, usable without a GPU).  tests/jpeg_enc_ref.py restates
 * the rules in numpy and is held to Pillow byte for byte; the files are held to both.
 *
 * Covered: 1 <= W, H <= 65535; quality 1 .. 100 (one per batch); sampling 1x1, 2x1, 2x2 (luma factors hs x vs; Pillow's subsampling 0, 1,
 * 2) per image; images of different sizes and samplings in one batch of 1 <= N <= 65535 with at most 2^31 - 1 blocks in all.
 *
 * THE RULES.
 *   1 Colour.   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;
 *               Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 *   2 Edges.    Luma: the last column and row replicated to whole blocks, ceil(W / 8) x ceil(H / 8) of them.  Chroma with hs = 2, in
 *               this order: the last column replicated at full resolution to 16 ceil(W / 16); for vs = 2 the last row once when H is
 *               odd; the downsample - 2x1: (a + b + bias) >> 1 with bias 0, 1, 0, 1, ... along the output row, 2x2:
 *               (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ...; then the last DOWNSAMPLED row replicated to whole blocks.
 *   3 Transform. Samples minus 128; libjpeg's accurate integer forward DCT (13 constant bits, 2 pass-1 bits, rows then columns, its
 *               rounding shifts; constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172); output times 8; int32.
 *   4 Quantisation.  Annex K tables; s = 5000 / q for q < 50, else 200 - 2 q; t = clip((base s + 50) / 100, 1, 255);
 *               coefficient = sign(v) ((|v| + 4 t) / (8 t)).
 *   5 Dummy blocks (luma blocks of the MCU grid beyond the component's own blocks; hs = 2 only): all AC terms zero; in a real block
 *               row the DC of the block to the left; in a dummy row the DC of the LAST block of the row above within the same MCU,
 *               which may itself be a right-edge dummy.
 *   6 Scan.     One interleaved scan, MCUs in raster order, inside an MCU the luma blocks row by row, then Cb, then Cr; a DC predictor
 *               per component; Annex K Huffman tables; a negative value travels as v - 1 in its low bits; F0 for each run of 16 zeros,
 *               00 ends a block unless its last coefficient is non-zero; bits most significant first; 00 after every FF data byte;
 *               the last byte filled with one-bits (and stuffed like any other), then FF D9.
 *   7 Headers.  SOI; APP0 JFIF 1.01, units 0, density 1x1, no thumbnail; two DQT of 67 bytes; SOF0; DHT DC0, AC0, DC1, AC1; SOS:
 *               FD_JPEG_ENC_HEADER_BYTES bytes whatever the image.
 *
 * THE CALLS, in order, for one batch:
 *   fd_jpeg_enc_layout  host.  In: width, height, hs, vs of every descriptor.  Out: their MCU grid, first block, first tile and the
 *                       worst-case sizes - a block takes at most FD_JPEG_ENC_BLOCK_BYTES bytes before stuffing (22 bits of DC and 63
 *                       times 26 bits of AC), a file at most out_cap = header + twice that + 2 - and *sizes.  The caller allocates
 *                       `work` (sizes.work_bytes, 16-byte aligned) and `out` (sizes.out_bytes).
 *   fd_jpeg_enc_encode  checks the table against the layout, copies it and the tables (quantisation, Huffman) to work, clears the
 *                       unstuffed streams, and launches, whatever N and the sizes are:
 *     A k_jpeg_enc_blocks  rules 1 to 5.  A wave takes 8 blocks, a lane one row of a block: it builds its 8 samples from the pixels
 *                       (colour, edge replication and the chroma downsample on the load), does the row pass in registers, passes the
 *                       block through LDS, does the column pass and the quantisation of one column, and the wave stores the int16
 *                       coefficients in zigzag order, 16 bytes a lane, in scan order, dummy blocks included (a dummy block runs its
 *                       source block's arithmetic and keeps the DC).
 *     B k_jpeg_enc_bits    a lane per block: the bits of its tokens, the DC against its predecessor of the same component.
 *     C k_jpeg_enc_scan    a workgroup per image: the exclusive scan of the bit counts, 64-bit, and the stream's length.
 *     D k_jpeg_enc_emit    a lane per block packs its tokens, 32 bits at a time, with integer atomic ORs on byte-swapped 32-bit words
 *                       of the cleared stream, bounds-checked against the image's room.
 *     E k_jpeg_enc_ffcount, k_jpeg_enc_scan again, k_jpeg_enc_stuff: the FF bytes of every FD_JPEG_ENC_TILE_BYTES tile of the filled
 *                       stream, their exclusive scan per image, and the stuffed bytes, FF D9 and one fd_jpeg_enc_result per image;
 *                       the files follow each other from byte 0 of out, each with FD_JPEG_ENC_HEADER_BYTES unwritten bytes in front.
 *                       SEVEN launches, one clear and two small uploads per batch.  Integer arithmetic and integer atomics only: two
 *                       calls give the same bytes.
 *   (download)          work[result_off ..): N fd_jpeg_enc_result; then out[0 .. sum of out_bytes) into pinned memory.
 *   fd_jpeg_enc_header  host, per file: the header bytes at the file's start. */
#define FD_JPEG_ENC_HEADER_BYTES 623
#define FD_JPEG_ENC_BLOCK_BYTES 208
#define FD_JPEG_ENC_TILE_BYTES 4096
typedef struct fd_jpeg_enc_desc {
    const void* src;                 /* DEVICE pixels, uint8 [H][W][3], contiguous */
    long first_block, blocks;        /* layout: the batch-wide index of the image's first block in scan order; its block count */
    long raw_off, raw_cap;           /* layout: the image's unstuffed stream inside work; its room (whole tiles) */
    long first_tile;                 /* layout: the batch-wide index of the image's first tile */
    long out_cap;                    /* layout: the worst-case size of the file */
    int width, height;
    int hs, vs;                      /* luma sampling factors: 1x1, 2x1 or 2x2 */
    int mcus_w, mcus_h;              /* layout */
    int reserved[4];
} fd_jpeg_enc_desc;
typedef struct fd_jpeg_enc_sizes {
    long blocks, tiles;              /* of the whole batch */
    long tab_off, coef_off, bits_off, pos_off, tile_off, tilepos_off, total_off;
    long result_off, result_bytes;   /* the download */
    long raw_off, raw_bytes;         /* the clear */
    long work_bytes;
    long out_bytes;                  /* the sum of out_cap, rounded up to 16 */
    long reserved;
} fd_jpeg_enc_sizes;
typedef struct fd_jpeg_enc_result {
    long out_off, out_bytes;         /* the file inside out, header included */
    long stream_bits;                /* before the fill and the stuffing */
    long stuffed;                    /* the 00 bytes added */
} fd_jpeg_enc_result;
int fd_jpeg_enc_quant_tables(int quality, unsigned short* zigzag /* [2][64]: luminance, chrominance, as a DQT segment holds them */);
int fd_jpeg_enc_header(int width, int height, int hs, int vs, int quality, unsigned char* dst, long dst_bytes);
int fd_jpeg_enc_layout(fd_jpeg_enc_desc* desc, int N, fd_jpeg_enc_sizes* sizes);
int fd_jpeg_enc_encode(void* work, long work_bytes, const fd_jpeg_enc_desc* desc, int N, int quality, unsigned char* out, long out_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDHIP_H */
