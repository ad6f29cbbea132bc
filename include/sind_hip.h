/* libsind_hip — C ABI of the MI355X-native DynaDetect + ORBextractor hot path.
 *
 * The reference (qimao7213/SInDSLAM) has no FFI layer: its boundary is two C++ classes,
 *   ORB_SLAM2::DynaDetect    (ORB_SLAM2/include/DynaDetect.h:95-131, src/DynaDetect.cc:1377-1666)
 *   ORB_SLAM2::ORBextractor  (ORB_SLAM2/include/ORBextractor.h:54-88, src/ORBextractor.cc:1043-1164)
 * called from Examples/RGB-D/rgbd_tum_noros.cc:106-107,135,138 and src/Frame.cc:308.  Each entry point below names
 * the reference member it replaces.  include/DynaDetect.h and include/ORBextractor.h are header-only C++ shims with
 * the reference's class names and signatures on top of this ABI.
 *
 * Conventions: plain pointers and sizes, caller-owned memory, row strides in BYTES, return 0 on success or a negative
 * SIND_E_* code (sind_last_error() gives the text), no exceptions cross the ABI.  A handle is bound to one GPU and
 * one HIP stream and is not thread-safe; use one handle per thread.  "_dev" entry points take DEVICE pointers
 * (inputs already resident in HBM) and are asynchronous on the handle's stream until sind_*_sync().
 */
#ifndef SIND_HIP_H
#define SIND_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SIND_OK 0
#define SIND_E_ARG (-1)
#define SIND_E_HIP (-2)
#define SIND_E_ALLOC (-3)
#define SIND_E_STATE (-4)
#define SIND_E_CAPACITY (-5)

const char* sind_last_error(void);
int sind_device_count(int* count);

/* ------------------------------------------------------------------------------------------------------------
 * Dense flow stage (state free).  Replaces, for B frame pairs at once on the 0.6-scaled grid:
 *   cv::optflow::createOptFlow_DeepFlow()->calc(I_n, I_prev, flow)      DynaDetect.cc:1031,1075,1127
 *   cv::VariationalRefinement::create()->calc(I_n, I_prev, flow)        DynaDetect.cc:1133-1143
 * Images: u8 [B][fh][fw] dense.  Flow: two planes u, v, f32 [B][fh][fw] (the reference's CV_32FC2 de-interleaved).
 */
typedef struct sind_flow sind_flow;
int sind_flow_create(int fw, int fh, int max_batch, int device, sind_flow** out);
int sind_flow_destroy(sind_flow* f);
int sind_flow_levels(sind_flow* f, int* widths, int* heights, int cap);          /* returns the level count */
int sind_flow_deepflow(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v);       /* host pointers */
int sind_flow_refine(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v);         /* host, u/v in-out */
int sind_flow_varref_f32(sind_flow* f, const float* i0, const float* i1, int w, int h, int B, float* u, float* v,
                         int fixed_point_iters, int sor_iters, float alpha, float delta, float gamma, float omega); /* host, one level */
int sind_flow_deepflow_dev(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v);   /* device pointers, async */
int sind_flow_refine_dev(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v);
int sind_flow_sync(sind_flow* f);
/* build-side option (BASELINE.json config 5, "3-level flow pyramid"; no reference counterpart -- OpenCV 4.2's DeepFlow never advances its
 * maxLayers counter): n > 0 keeps only the finest n levels of the 0.95 pyramid, the flow starts from zero at the coarsest of them; 0 = all */
int sind_flow_set_max_levels(sind_flow* f, int n);
/* per handle: on != 0 (default) runs every pyramid level that is one workgroup's work (<= 4096 pixels) -- warp, coefficients, SOR, W += dW and the up-sampling, for all
 * such levels of a DeepFlow pyramid -- in ONE launch (k_coarse_chain); 0 = per-stage kernels on every level (cross-check, A/B timing).  Same bits either way. */
int sind_flow_set_coarse_chain(sind_flow* f, int on);
/* per handle: on != 0 (default) solves a tiled level whose tiles all find a compute unit of their own (few images per launch: the launch is latency-bound) with 1024-thread
 * tiles and up to 13 iterations per launch on deeper halos (k_sor_tile); 0 = the 512-thread tiles / streaming kernel at every batch size.  Same bits either way. */
int sind_flow_set_latency_tiles(sind_flow* f, int on);
/* per handle: on != 0 (default) makes the transition between two pyramid levels -- W += dW, the bilinear up-sampling / 0.95 and the next level's warp, average and temporal
 * difference -- one launch (k_level_up) instead of three; 0 = the three kernels (cross-check).  Same bits either way. */
int sind_flow_set_level_up(sind_flow* f, int on);
/* solver variant of THIS handle (every variant returns the same bits; nothing here is process-wide).  mode 4 = fused register-resident SOR with 1x8 pixel strips, divisions
 * through a reciprocal formed on the fly (hardware estimate + one Newton step, then Markstein's correction; default: 5 iterations per launch on 64 x 64 tiles), 5 = the
 * streaming kernel on every level it fits, 6 = the one-wave pipeline on every level beyond one workgroup, 0 = one launch per colour (cross-check).  fuse = iterations per
 * launch on tiled levels (1 .. 12, default 5); tile_w x tile_h = extended tile (tile_w * tile_h / 8 threads).  sind_flow_set_sor keeps the round-1 argument list (tile height 64). */
int sind_flow_set_sor(sind_flow* f, int mode, int fuse, int tile_w);
int sind_flow_set_sor_tiled(sind_flow* f, int mode, int fuse, int tile_w, int tile_h);
/* streaming solver: at most `cap` workgroups per launch, each taking several (column strip, image) items in turn (persistent workgroups); 0 = one workgroup per item.
 * Same results.  See DESIGN.md 3.1-12 for when it pays. */
int sind_flow_set_solver_workgroups(sind_flow* f, int cap);
/* one-wave row pipelines (k_sor_wave, flow_wave.hip) for the levels and batch sizes that would otherwise go to the streaming kernel: on != 0 (default) / 0 = k_sor_stream;
 * target_items = waves a launch should have (row bands are cut until it does; 0 keeps the default), bands > 0 = exactly that many row bands (tests); on = 2 / 3 / 4 additionally selects 1 / 2 / 3 rows
 * in flight per wave (A/B timing; default 2).  Mode 6 of
 * sind_flow_set_sor_tiled runs the kernel on every level beyond one workgroup at any batch size.  Same bits either way. */
int sind_flow_set_wave_solver(sind_flow* f, int on, int target_items, int bands);
/* how k_sor_wave cuts a w x h level of B pairs (host arithmetic only, no GPU needed): out = {column strips, kept columns per strip, row bands, kept rows per band}.  A strip works on
 * 128 columns -- its kept ones plus 10 on every side that is not an image border --, a band on its kept rows plus 10 on every cut side. */
int sind_flow_wave_layout(int w, int h, int B, int target_items, int bands, int out[4]);
/* k_sor_wave cuts its column strips over groups of `group` consecutive images laid side by side (image i of a group at the columns [i * period, i * period + w) of a virtual
 * row; the period is even and > w, the columns between two images stay zero): 0 = the group size of 1 .. 32 that needs the fewest waves per launch (default), 1 = every image
 * on its own (sind_flow_wave_layout's launch), n = exactly min(n, images of the launch) (tests).  Same bits either way. */
int sind_flow_set_wave_pack(sind_flow* f, int group);
/* the layout under that setting (host arithmetic only): out = {images per group, period, column strips per GROUP, kept columns per strip, row bands, kept rows per band}.  The
 * strips are sind_flow_wave_layout's uniform ones over the (group - 1) * period + w columns of the virtual row; the bands are sind_flow_wave_layout's. */
int sind_flow_wave_pack_layout(int w, int h, int B, int target_items, int bands, int group, int out[6]);
/* which kernel solves a w x h level of B pairs with `total` SOR iterations under the given settings (host arithmetic only, no GPU needed; for tests of the policy).  The settings are
 * the setters' arguments: mode / fuse / tile_w / tile_h as in sind_flow_set_sor_tiled, wave as `on` of sind_flow_set_wave_solver, stream_min_b = images per launch from which the
 * large levels get their own solver (80 in every handle), latency_tiles and coarse_chain as in their setters.  out[0] = kernel: 0 k_coarse_chain (the whole level in one launch),
 * 1 k_sor_color (two launches per iteration), 2 k_sor_tile, 3 k_sor_fused on the whole level in one workgroup, 4 k_sor_wave, 5 k_sor_stream, 6 k_sor_fused on tiles; out[1] = n = number
 * of launches (iterations for kernel 1); out[2 .. 2 + n) = iterations of each.  SIND_E_ARG: bad arguments, cap < 2 + n, or a level / tile that k_sor_fused cannot hold. */
int sind_flow_sor_plan(int mode, int fuse, int tile_w, int tile_h, int wave, int stream_min_b, int latency_tiles, int coarse_chain, int w, int h, int B, int total, int* out, int cap);
/* coefficient kernel: 1 = k_coef_lanes (neighbours from lanes, short sqrt / c / sqrt forms that are correctly rounded for arguments >= 2^-96; default), 2 = k_coef_lanes with the compiler's IEEE sqrt and c / sqrt
 * (every variant divides by the gradient norms through their reciprocals: correctly rounded for numerators >= 2^-100 or zero, the IEEE division below; sind_debug_div_scan),
 * 0 = k_coef (neighbours from memory), 3 = variant 1 with its tiles in plain grid order over the XCDs (A/B timing: by default the tiles of a pair share an XCD's L2).  Same results. */
int sind_flow_set_coef_kernel(sind_flow* f, int variant);
/* HIP-event timing of everything enqueued on the handle's stream between begin and end (bench.py roofline leg) */
int sind_flow_timer_begin(sind_flow* f);
int sind_flow_timer_end(sind_flow* f, float* milliseconds);

/* ------------------------------------------------------------------------------------------------------------
 * ORBextractor.  Replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:54-88):
 *   ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)     src/ORBextractor.cc:410-470  -> sind_orb_create
 *   operator()(image, mask, keypoints, descriptors)                         src/ORBextractor.cc:1043-1164 -> sind_orb_extract
 *   GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / Get(Inverse)ScaleSigmaSquares -> sind_orb_tables
 *   public member mvImagePyramid (read by Frame::ComputeStereoMatches)                     -> sind_orb_pyramid
 * sind_keypoint mirrors cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id).
 * mask: the dilated imgDyna (255 = dynamic) or NULL; "empty image -> silent return" maps to n = 0 with SIND_OK.
 */
typedef struct sind_orb sind_orb;
typedef struct sind_keypoint { float x, y, size, angle, response; int octave, class_id; } sind_keypoint;
int sind_orb_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast, int device, sind_orb** out);
int sind_orb_destroy(sind_orb* o);
int sind_orb_reserve(sind_orb* o, int width, int height, int max_batch);   /* optional: pre-size the workspaces */
int sind_orb_extract(sind_orb* o, const uint8_t* gray, int width, int height, int stride, const uint8_t* mask_or_null, int mask_stride,
                     sind_keypoint* kps, int cap, int* n, uint8_t* desc /* cap x 32 */);
/* B images [B][height][width] dense (host); masks [B][height][width] or NULL; outputs [B][cap], n[B], desc [B][cap][32] */
int sind_orb_extract_batch(sind_orb* o, const uint8_t* gray, int width, int height, int B, const uint8_t* masks_or_null,
                           sind_keypoint* kps, int cap, int* n, uint8_t* desc);
int sind_orb_tables(sind_orb* o, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2, int* features_per_level, int* umax16);
/* padded pyramid level of frame `frame` of the last call (19-px REFLECT_101 border): copies (w+38)*(h+38) bytes */
int sind_orb_pyramid(sind_orb* o, int frame, int level, uint8_t* out, int* w, int* h);
/* parity-test access to the stage outputs of the last call: cell-wise FAST keypoints of one level (x, y, response triplets,
 * coordinates relative to the 16-px min border) and the octree survivors with their orientation before mask erasure */
int sind_orb_debug_fast(sind_orb* o, int frame, int level, float* xyr, int cap);
int sind_orb_debug_selected(sind_orb* o, int frame, sind_keypoint* kps, int cap, uint8_t* desc);
/* the 7x7 sigma-2 Gaussian-blurred level BRIEF reads, frame `frame` of the last call: copies the w*h interior, dense */
int sind_orb_debug_blurred(sind_orb* o, int frame, int level, uint8_t* out, int* w, int* h);

/* ------------------------------------------------------------------------------------------------------------
 * DynaDetect.  Replaces ORB_SLAM2::DynaDetect (include/DynaDetect.h:95-131):
 *   DynaDetect(imgLast, imgLastLast, fx, fy, cx, cy, depthScale)   DynaDetect.h:98-126         -> sind_dyna_create + sind_dyna_prime
 *   DetectDynaArea(img, imgDepth, imgDyna, imgLabel, nImg)         DynaDetect.cc:1377-1666     -> sind_dyna_detect
 * img: CV_8UC3 BGR, imgDepth: CV_16UC1 (raw units = metres * depthScale), imgDyna: CV_8UC1 0 invalid / 125 static /
 * 255 dynamic, imgLabel: CV_8UC1 0 invalid, 1..n.  The reference's imshow / waitKey / stdout side effects are dropped.
 * Like the reference class the handle carries inter-frame state and is not re-entrant.
 */
typedef struct sind_dyna sind_dyna;
int sind_dyna_create(int width, int height, float fx, float fy, float cx, float cy, float depth_scale, int device, sind_dyna** out);
int sind_dyna_destroy(sind_dyna* d);
int sind_dyna_set_flow_max_levels(sind_dyna* d, int n);      /* see sind_flow_set_max_levels */
int sind_dyna_timing(sind_dyna* d, double ms12[12], int reset); /* mean ms per detect call: upload, dense flow, wait for the depth half, flow masks + fusion, depth half, whole call;
                                                                    then the tail's stages: flow masks, k-means, label preparation, CalOccluded, SegAndMerge, fusion; returns calls */
/* summed milliseconds of the tail's sub-stages since the last reset (dyna.hpp t_fine: CalOccluded 0 gpu + d2h, 1 pack, 2 end points, 3 PEAC host parts, 4 contour filter, 5 close;
 * SegAndMerge 6 pieces, 7 alloc, 8 rag (h2d, kernels, d2h, wait), 9 merge, 10 sort + paint + pack, 11 h2d enqueue, 12 - 16 inside pieces: open, contours, masks, lianjie, centre; 20 - 23 flow masks on
 * the host: weights, sort + wait, homography, pack; 24 - 27 fusion) */
int sind_dyna_timing_fine(sind_dyna* d, double ms40[40], int reset);
int sind_dyna_set_debug(sind_dyna* d, int on);               /* on: keep the intermediate images sind_dyna_debug reports (costs four flow-sized copies per frame); default off */
int sind_dyna_set_overlap(sind_dyna* d, int on);             /* default on: the depth half of a frame (k-means, CalOccluded, SegAndMerge) runs beside its dense flow, as the reference's
                                                                 flow thread runs beside the segmentation (DynaDetect.cc:1396-1398); 0 = one after the other; same results */
int sind_dyna_prime(sind_dyna* d, const uint8_t* bgr_last, const uint8_t* bgr_lastlast, int stride);
int sind_dyna_detect(sind_dyna* d, const uint8_t* bgr, int bgr_stride, const uint16_t* depth, int depth_stride,
                     uint8_t* dyna_out, uint8_t* label_out, int n_img);
/* caller-side 15x15 elliptical dilation of imgDyna before tracking (Examples/RGB-D/rgbd_tum_noros.cc:108,138), in place */
int sind_dyna_dilate15(sind_dyna* d, uint8_t* dyna_inout);
/* parity-test access to the stage outputs of the last sind_dyna_detect call; any pointer may be NULL.
 * flow_*: f32 planes (u then v), deep/refined at the 0.6 grid, full at width x height.  thr = {maxError, otsu, triangle, low, high}.
 * info = {largeMotion, nPairs, nPieces}. */
int sind_dyna_debug(sind_dyna* d, float* flow_deep, float* flow_refined, float* flow_full, double* H9, float* thr5, int* hist256,
                    uint8_t* mask_low, uint8_t* mask_high, uint8_t* kmeans_label, float* centers36, uint8_t* occ1, uint8_t* occ2,
                    uint8_t* total_area, uint8_t* grad_edge, uint8_t* plane_contours, int* info3);

/* parity-test access to the k-means centre sums: out = the FP32 value of  acc = 0; for (i) acc += x[i]  (round to nearest even, exactly cv::kmeans'
 * centre accumulation, kmeans.cpp) computed by the wave-parallel window arithmetic of k_km_seqsum (csrc/depth_kmeans.hip) */
int sind_debug_seqsum(const float* x, int n, int device, float* out);
/* k-means pyramid levels of at most n points (default 81920 = the three coarse levels at 640 x 480) of a batch of at least b frames (default 32: the batched rounds of a
 * many-stream step) run every pass in ONE launch, one workgroup per frame (k_km_level_fused); n = 0: the per-pass kernels everywhere.  Same labels and centres bit for bit
 * (tests/test_kmeans_fused_gpu.py).  They set the DEFAULTS that handles created AFTERWARDS copy; an existing handle keeps what it was created with (parity tests, A/B timing). */
int sind_debug_set_kmeans_fused_max(int n);
int sind_debug_set_kmeans_fused_min_batch(int b);
/* exhaustive check of the short forms: for every float significand and the binary exponents exp_lo..exp_hi (>= -96), out[0] = arguments whose short-form square root differs
 * from sqrtf, out[1] = quotients numer[k] / b through the reciprocal (hardware estimate + Newton step + Markstein's correction) that differ from the IEEE division */
int sind_debug_coef_math_scan(int device, int exp_lo, int exp_hi, const float numer[3], unsigned long long out[2]);
/* exhaustive check of the solver's division: for every float significand and the binary exponents exp_lo..exp_hi, out[0] = reciprocals (hardware
 * estimate + one Newton step) that differ from the correctly rounded 1 / a, out[1] = quotients through that reciprocal (Markstein) that differ
 * from the IEEE division (16 numerators per divisor), out[2] = smallest failing significand (all ones if none) */
int sind_debug_rcp_scan(int device, int exp_lo, int exp_hi, unsigned long long out[3]);
/* the same two quotients (sor_div of the solver kernels, kc_div of the coefficient kernels) against the IEEE division BELOW the range of the two scans above, where the
 * residual of Markstein's correction is no longer exact: every divisor significand x the divisor exponents -7 .. 14 x one numerator of random sign and significand per binary
 * exponent from -149 (the smallest denormal) up to the divisor's exponent - 40, and the numerators +0 and -0.  counts[0] / counts[1] = quotients of sor_div / kc_div that differ,
 * counts[2] = those of them with a zero numerator, *max_exp = the largest numerator exponent of a mismatch (-1000: none), by_exp (optional) = mismatches of both helpers at the
 * numerator exponents -149 .. -26 */
int sind_debug_div_scan(int device, unsigned long long counts[3], int* max_exp, unsigned long long by_exp[124]);

/* parity-test access to the residual-threshold kernel (Otsu + Triangle of cv::threshold and the clamping of DynaDetect.cc:1309-1367 from a 256-bin
 * histogram): hist = n blocks of 257 words (counts, then the float bits of the maximal residual), res = n blocks of 261 words (the 257 input words,
 * then lo, hi, otsu, triangle as floats; variant 0 writes only n x 4 floats, packed at the start of res).  variant 0 = serial one-thread reference
 * kernel, 1 = one-wave kernel, 2 = one-wave kernel in its production form, which clears the working histogram: the first 257 words of every result
 * block then hold the cleared words.  mu1 (optional, variants 1 / 2): n x 256 values of Otsu's running class mean, the one rounding chain with a division. */
int sind_debug_flow_thresholds(const int* hist, int n, int width, int height, int variant, int device, int* res, double* mu1);
/* parity-test access to the large-motion test (DynaDetect.cc:1081-1114) without DeepFlow and without the sign flip: B flow fields (host f32 [B][fh][fw] each, fw x fh
 * the 0.6-scaled grid of a W x H frame) go through the production launch of the magnitude maximum and histogram with batch B and the host decision the dense flow calls.
 * flags: B values (0 / 1); hist (optional): B x 256 counts; maxflow (optional): B maxima of |flow|; end (optional): B x 2 = endFlow, endFlow2. */
int sind_debug_large_motion(const float* u, const float* v, int B, int fw, int fh, int W, int H, int device, int* flags, int* hist, float* maxflow, int* end);
/* parity-test access to the batched flow-mask stage (csrc/flow_mask.hip: k_residual_mag_frames, k_mag_hist_frames, k_flow_thresholds_frames,
 * k_flow_mask_bits_frames): n frames of dense flow (host f32 [n][height][width] each) and n homographies (row-major 3 x 3 doubles) go through the four
 * batched launches and, in the same call, frame by frame through the per-frame kernels.  Both sets come back: masks as u8 [n][height * width] (low: 0 / 128,
 * high: 0 / 255; the batched bit masks are expanded on the host) and result blocks [n][261] (256 histogram counts, the float bits of the maximal residual,
 * lo, hi, otsu, triangle as floats).  width must be a multiple of 64. */
int sind_debug_flow_masks_batch(const float* u, const float* v, const double* homographies, int n, int width, int height, int device,
                                uint8_t* low_batch, uint8_t* high_batch, int* res_batch, uint8_t* low_frame, uint8_t* high_frame, int* res_frame);
/* the same, with the intermediate images of both paths and a way into the per-frame mask kernel's narrow path: byte_offset (0..15) moves the per-frame u8 residual and both
 * per-frame mask planes that many bytes off their 16-byte alignment (0: the production layout, 16 pixels per thread; otherwise k_threshold_masks_dev takes one pixel per
 * thread).  mag_batch / mag_frame (optional): the FP32 residual [n][height * width] of the batched and the per-frame kernels; magu8_batch / magu8_frame (optional): its
 * u8 normalisation. */
int sind_debug_flow_masks_stage(const float* u, const float* v, const double* homographies, int n, int width, int height, int device,
                                uint8_t* low_batch, uint8_t* high_batch, int* res_batch, uint8_t* low_frame, uint8_t* high_frame, int* res_frame,
                                int byte_offset, float* mag_batch, uint8_t* magu8_batch, float* mag_frame, uint8_t* magu8_frame);

/* parity-test access to the GPU region grow of the PEAC plane refinement (AHCPlaneFitter.hpp:546-601 floodFill; csrc/peac_kernels.hip): n depth frames
 * (host u16 [n][height][width]) -> membership map per pixel (plane index or -1) from ONE kernel launch over all frames (member_gpu) and from the host
 * statement of the same FIFO (member_host), both int8 [n][height * width]; pair_* [n][127 * 127]: which planes met (row stride = the frame's plane count);
 * status [n][4] = kernel status (0 ok, 1..3 capacity errors, 4 skipped), BFS levels, seeds processed, planes. */
int sind_debug_peac_grow(const uint16_t* depth, int n, int width, int height, float fx, float fy, float cx, float cy, float depth_scale, int device,
                         int8_t* member_gpu, int8_t* member_host, uint8_t* pair_gpu, uint8_t* pair_host, int* status);

/* parity-test access to the GPU front of CalOccluded (DynaDetect.cc:429-482) and the depth normalisation of the region-adjacency stage (DynaDetect.cc:765-768) through the
 * production launchers (csrc/depth_edges.hip: k_median5_u16, k_max_u16, k_grad_edge, k_morph_e4, k_depth_norm): n depth frames (host u16 [n][height][width], 1 <= n <= 64,
 * 7 <= width, height <= 4096).  n == 1 takes the single-frame forms of the drop-in path, n >= 2 the batched forms of the pipeline.  Per frame: filt = medianBlur(5) (u16),
 * maxima [n][2] = {maximum of filt, maximum of the raw frame}, edge_pre / edge = the gradient edge before / after MORPH_OPEN with the 4 x 4 ellipse, total_area, depth_n = the
 * 8-bit normalised depth; images are [n][height][width]. */
int sind_debug_depth_front(const uint16_t* depth, int n, int width, int height, float depth_scale, int device,
                           uint16_t* filt, unsigned* maxima, uint8_t* edge_pre, uint8_t* edge, uint8_t* total_area, uint8_t* depth_n);

/* parity-test access to the bit-plane dilation used by the region-adjacency stage (7x7 ellipse on 64-pixel words, cv::dilate semantics):
 * planes / out are host arrays [nplanes][height][ceil(width / 64)] of 64-bit words, bit i of word k = pixel 64 k + i. */
int sind_debug_dilate_planes(const unsigned long long* planes, int nplanes, int width, int height, int n, int device, unsigned long long* out);
/* parity-test access to the batched RAG stage against the per-frame one: n frames (1..64, width a multiple of 64) with pieces[i] pieces each (1..254).  planes: host
 * words, frame after frame, per frame [2][pieces[i]][height][width / 64] (piece planes, then connection planes); occ2 / depth_n: [n][height][width] u8.  Both forms
 * write, frame after frame, the stage's five outputs [overlap C*C][overlapPlane C*C][ljOverlap C*C][ljArea C][hist C*256] (C = pieces[i]) into out_batch / out_frame:
 * the batched one through launch_rag_frames as ONE chunk, the per-frame one through the kernels of the unbatched tail. */
int sind_debug_rag_batch(const unsigned long long* planes, const int* pieces, const uint8_t* occ2, const uint8_t* depth_n, int n, int width, int height, int device,
                         int* out_batch, int* out_frame);

/* ------------------------------------------------------------------------------------------------------------
 * Batched multi-stream pipeline: S independent camera streams x T consecutive frames per step through
 * DynaDetect + 15x15 dilation + ORBextractor, i.e. the body of the frame loop of Examples/RGB-D/rgbd_tum_noros.cc:110-170
 * for S sequences at once.  The state-free stages (gray, resize, dense flow, ORB pyramid/FAST/orientation/BRIEF) are
 * batched over all S*T frames; the stateful tail of each stream runs in frame order on its own host thread + HIP stream.
 * A stream is exactly one reference DynaDetect instance: results equal S sequential single-stream runs.
 * Layouts (dense): bgr [S][T][H][W][3] u8, depth [S][T][H][W] u16, dyna/label/mask [S][T][H][W] u8,
 * kps [S][T][cap], nkp [S][T], desc [S][T][cap][32].  "_dev" takes DEVICE input pointers (frames already in HBM);
 * outputs are always host pointers (they feed the host-side tracker).
 */
typedef struct sind_pipe sind_pipe;
typedef struct sind_pipe_config {
    int width, height; float fx, fy, cx, cy, depth_scale;
    int nfeatures; float scale_factor; int nlevels, ini_th_fast, min_th_fast;
    int orb_gray_rgb_order;      /* 1: ORB gray uses RGB2GRAY on the BGR buffer (Camera.RGB: 1, src/Tracking.cc:246-251), 0: BGR2GRAY */
    int streams, frames_per_step, device;
    int host_threads;            /* 0 = library default (2 x the CPU share of the process) */
    int flow_max_levels;         /* 0 = the reference's full DeepFlow pyramid; n > 0: finest n levels only (see sind_flow_set_max_levels) */
    int flow_slices;             /* dense-flow slices of a step that run concurrently on their own streams: 0 = by step size (default), 1..4 fixed; same results */
    int flow_opts_off;           /* A/B switches, same results: bit 0 = no k_coarse_chain (see sind_flow_set_coarse_chain), bit 1 = no k_sor_tile (see sind_flow_set_latency_tiles), bit 2 = no k_level_up (see sind_flow_set_level_up), bit 3 = k_sor_stream instead of k_sor_wave (see sind_flow_set_wave_solver), bit 4 = a round's k-means waits for the whole tails of the frame before (not only for their depth halves), bits 8.. = target_items of sind_flow_set_wave_solver; 0 = defaults */
} sind_pipe_config;
int sind_pipe_create(const sind_pipe_config* cfg, sind_pipe** out);
int sind_pipe_destroy(sind_pipe* p);
int sind_pipe_prime(sind_pipe* p, int stream, const uint8_t* bgr_last, const uint8_t* bgr_lastlast);          /* host pointers */
int sind_pipe_process(sind_pipe* p, const uint8_t* bgr, const uint16_t* depth, uint8_t* dyna, uint8_t* label, uint8_t* mask_dilated,
                      sind_keypoint* kps, int cap, int* nkp, uint8_t* desc);                                    /* host inputs */
int sind_pipe_process_dev(sind_pipe* p, const uint8_t* bgr_dev, const uint16_t* depth_dev, uint8_t* dyna, uint8_t* label,
                          uint8_t* mask_dilated, sind_keypoint* kps, int cap, int* nkp, uint8_t* desc);          /* device inputs */
/* Software-pipelined form: phase A (GPU batch) of the submitted step overlaps with phase B (per-stream tails) of the previously
 * submitted one.  The output pointers of call i receive the results of step i-1 (*have_output = 0 on the first call);
 * sind_pipe_flush drains the last step.  Device inputs only need to stay valid until the call returns. */
int sind_pipe_submit_dev(sind_pipe* p, const uint8_t* bgr_dev, const uint16_t* depth_dev, uint8_t* dyna, uint8_t* label, uint8_t* mask_dilated,
                         sind_keypoint* kps, int cap, int* nkp, uint8_t* desc, int* have_output);
int sind_pipe_flush(sind_pipe* p, uint8_t* dyna, uint8_t* label, uint8_t* mask_dilated, sind_keypoint* kps, int cap, int* nkp, uint8_t* desc,
                    int* have_output);
/* Schedule of the synchronous step (sind_pipe_process / _process_dev): on != 0 runs the flow-independent half of every tail (depth
 * k-means, SegAndMerge; reference DynaDetect.cc:1410-1551) underneath the dense flow instead of after it.  Results are identical;
 * default off (environment SIND_DEPTH_AHEAD=1 turns it on at create), see DESIGN.md 3.1 item 7 for the measurement.  It also applies to
 * sind_pipe_submit_dev: the depth chain of step i+1 then runs next to the flow chain of step i -- the schedule of the in-order
 * ("exact") single-sequence mode (streams = 1), whose rate is 1 / max(depth-chain, flow-chain latency per frame). */
int sind_pipe_set_depth_ahead(sind_pipe* p, int on);
/* Inter-frame state of one stream (reference DynaDetect.h:172-178: imgDynaLast, imgLabelLast, imgMaskHighErrorLast, plus the k-means
 * warm labels of DynaDetect.cc:374-395; rolled at DynaDetect.cc:1660-1664) as an opaque blob of sind_pipe_state_bytes() bytes.  Lets one
 * long sequence continue on another handle or rank exactly where this one stopped (phase A sharded, phase B strictly in
 * frame order).  get: nothing may be pending.  set: after sind_pipe_prime (which resets the state); allowed while a step submitted
 * WITHOUT depth-ahead waits for its tails -- submit (phase A), receive the predecessor's state, set, flush. */
size_t sind_pipe_state_bytes(sind_pipe* p);
int sind_pipe_get_state(sind_pipe* p, int stream, uint8_t* buf, size_t n);
int sind_pipe_set_state(sind_pipe* p, int stream, const uint8_t* buf, size_t n);
/* Chunked sequences (one long sequence cut into contiguous chunks, one per stream; driver: sindslam_amd/sequence.py).  A chunk that starts in
 * the middle of the sequence rebuilds the inter-frame state in a few warm-up frames; whether the rebuilt state IS the state the sequential loop
 * (rgbd_tum_noros.cc:110-170) would have carried there is decided by comparing fingerprints: every output of a frame is a deterministic function of the
 * input frames and the state before it, so equal states after frame q mean equal results on every later frame.
 *   sind_pipe_set_state_hashing(on): every tail leaves a 128-bit fingerprint of its rolled state (DynaDetect.cc:1660-1664) per frame.
 *   sind_pipe_get_state_hashes: the fingerprints of the step whose results were returned last, [streams][frames_per_step][2] (0, 0 = frame not processed).
 *   sind_pipe_set_active_frames(n[streams]): in the NEXT step only, the stateful tail of stream s runs for its first n[s] frames (0..frames_per_step); the
 *     state of the stream then is the state after frame n[s] - 1 -- a chunk can end, and its state be taken with sind_pipe_get_state, in the middle of a
 *     step.  Outputs of the skipped frames are not written.  The state-free work still covers all frames, and the stream's gray history ends up at the
 *     step's last frame: prime the stream again before it processes anything else.  NULL = all frames.  Not available with depth-ahead. */
int sind_pipe_set_state_hashing(sind_pipe* p, int on);
int sind_pipe_get_state_hashes(sind_pipe* p, uint64_t* out, size_t count);
/* Which pairs of the step whose results were returned last took the reference's second DeepFlow pass (flow(n, n-1) instead of flow(n, n-2), DynaDetect.cc:1121-1131):
 * streams x frames_per_step flags (0 / 1), pair k = stream * frames_per_step + frame.  Read-only; the flag depends on the frames alone, so a ragged step has all of them. */
int sind_pipe_large_motion(sind_pipe* p, int* flags, int cap);
/* Which schedule the stateful tails of that step took: 0 = one chain per stream over whole tails, 1 = chains over flow halves (depth-ahead), 2 = two chains per stream
 * (ragged / replayed steps with few live streams), 3 = rounds, 4 = split rounds.  Read-only; SIND_E_STATE before the first step.  The results do not depend on it. */
int sind_pipe_last_schedule(sind_pipe* p, int* kind);
int sind_pipe_set_active_frames(sind_pipe* p, const int* frames_per_stream);
/* Retained steps: the repair runs of the chunked mode re-run only the stateful 1 % of a frame.  sind_pipe_reserve_retained(n) sets buffers for n steps aside
 * (device: flow, depth, plane-edge mask, normalised depth; page-locked host: depth, sample-grid flow); sind_pipe_retain_next(tag) keeps the phase-A outputs
 * (dense flow, depth copies, ORB front results, CalOccluded results; reference DynaDetect.cc:1023-1147, :429-642, ORBextractor.cc:1043-1151) of the NEXT
 * submitted step under `tag` once its tails have run; sind_pipe_replay(tag, first, last, outputs) runs the tails (DynaDetect.cc:315-420, 653-1018, 1163-1367,
 * 1553-1664 + dilation + mask filter of the keypoints) of frames [first[s], last[s]) of that step again for every stream, from the state the stream holds now
 * (sind_pipe_set_state) -- nothing may be pending; outputs in the step layout, only the frames that ran are written; sind_pipe_release_retained(tag) hands the
 * buffers back (tag < 0: all).  Not available with depth-ahead.  The reserve is EXACTLY n sets: unused sets beyond n are freed by the call (n = 0 frees all unused ones),
 * a call that fails for lack of memory keeps the sets it had completed -- call again with a smaller n to give the surplus back. */
int sind_pipe_reserve_retained(sind_pipe* p, int steps);
int sind_pipe_retain_next(sind_pipe* p, int tag);
int sind_pipe_replay(sind_pipe* p, int tag, const int* first, const int* last, uint8_t* dyna, uint8_t* label, uint8_t* mask_dilated,
                     sind_keypoint* kps, int cap, int* nkp, uint8_t* desc);
int sind_pipe_release_retained(sind_pipe* p, int tag);
/* A ragged or replayed step in which at most n streams have frames runs them as two chains per stream -- the depth half (k-means from the previous frame's merged
 * labels, SegAndMerge) ahead of the flow half (flow masks, fusion, dilation, keypoint filter), own k-means launches, no round barrier -- instead of batched rounds
 * (default 12; 0 = always rounds).  Same results; for a handful of streams on an otherwise idle GPU a frame costs max(depth, flow) instead of a whole round (the slow
 * runners of a repair: 1.10 -> 0.70 s on the Bonn-shaped stream, profiles/r04/repair_latency.txt). */
int sind_pipe_set_chain_max_streams(sind_pipe* p, int n);
/* per-stage wall times of the last step in milliseconds: {front_gray, dense_flow, orb_front, host_upload (sind_pipe_process only, else 0), tails, total},
 * plus HIP-event statistics of the flow solver of the large levels (see sind_pipe_sor_other_stats): sor_launches, sor_ms (sum of event-bracketed SOR launch groups),
 * sor_alg_bytes (algorithmic bytes those launches cover: 44 B per pixel per red+black iteration) */
int sind_pipe_stats(sind_pipe* p, double* stage_ms6, long long* sor_launches, double* sor_ms, double* sor_alg_bytes);
/* flow-solver statistics of the last step when the batch is cut into concurrent slices (one HIP stream each): launches and algorithmic
 * bytes of all slices, sum_ms = sum of the event-bracketed launch groups, union_ms = time during which at least one slice had solver
 * launches in flight (union of those intervals on a common event time base), slices = number of concurrent streams */
int sind_pipe_sor_stats(sind_pipe* p, long long* launches, double* sum_ms, double* union_ms, double* alg_bytes, int* slices);
/* since round 5 the two calls above count the launch groups of the solver of the LARGE levels only, at 80 images per launch and more (k_sor_wave by default, k_sor_stream with
 * sind_flow_set_wave_solver(f, 0, ...) / flow_opts_off bit 3: the kernel bench.py's roofline object describes); this one reports the other solver launches of the step (tiles, one-workgroup levels outside k_coarse_chain, whose solver phases are not separate launches) */
int sind_pipe_sor_other_stats(sind_pipe* p, long long* launches, double* sum_ms, double* alg_bytes);
/* last sind_pipe_submit(_dev): time the call still waited for the previous step's tails after its own phase A had finished (0 = hidden) */
int sind_pipe_tail_wait_ms(sind_pipe* p, double* ms);
/* how the handle sized its host side: {CPU share of this process (cores), pool workers, CPU tokens (max), cores the process may run on, cgroup cpu.max quota in
 * cores or -1, ranks sharing the node (LOCAL_WORLD_SIZE)}.  share = min(cores, quota) / ranks, at least 4, at most 16. */
int sind_pipe_host_info(sind_pipe* p, int* out6);
/* several handles driven concurrently on one GPU share the process's CPU share: give each its part (cores >= 1; tokens of the pool tasks and the
 * CalOccluded runners follow; the worker threads stay as created) */
int sind_pipe_set_cpu_share(sind_pipe* p, int cores);
int sind_pipe_mask_bytes(sind_pipe* p, size_t* bytes);      /* size of one step's dyna / label / mask array: streams * frames_per_step * height * width */

/* ------------------------------------------------------------------------------------------------------------
 * The multi-GPU collective of the path: frames of a sequence shard across the GPUs of a node, one process per GPU, and the per-frame
 * dynamic masks are gathered with ONE ncclAllGather (RCCL, xGMI) per pipeline step.  No other collective exists: the path shards by frame.
 * Rank 0 calls sind_comm_unique_id and passes the 128 bytes to the other ranks out of band (the application's own channel); every rank then calls
 * sind_comm_create(id, rank, world, device).  sind_pipe_gather_masks sends the `dyna` array a step returned (host memory) and receives all ranks' arrays in
 * rank order into all_dev (device memory, world * sind_pipe_mask_bytes) and, if not NULL, all_host.  RCCL is loaded at first use (dlopen): a box
 * without it still loads the library and gets SIND_E_STATE from these calls. */
typedef struct sind_comm sind_comm;
int sind_comm_unique_id(void* id128, size_t bytes);
int sind_comm_create(const void* id128, int rank, int world, int device, sind_comm** out);
int sind_comm_destroy(sind_comm* c);
int sind_comm_rank(const sind_comm* c);
int sind_comm_world(const sind_comm* c);
int sind_comm_allgather_u8(sind_comm* c, const uint8_t* local_host, size_t bytes, uint8_t* all_dev, uint8_t* all_host_or_null);
/* one hand-over along the chain of ranks as one RCCL group: `bytes` bytes of host memory to rank `to` (-1: nothing to send) and as many from rank `from` (-1: nothing) */
int sind_comm_sendrecv_u8(sind_comm* c, const uint8_t* send_host, int to, uint8_t* recv_host, int from, size_t bytes);
int sind_pipe_gather_masks(sind_pipe* p, sind_comm* c, const uint8_t* dyna_host, uint8_t* all_dev, uint8_t* all_host_or_null);
/* Where the PEAC region grow of CalOccluded (AHCPlaneFitter.hpp:546-601) runs: `quarters` of every four frames on the GPU (k_peac_grow, one compute unit for
 * a few ms per frame), the others on a host core; the results are bit-identical, the share only moves load between the GPU and the host.  -1 (default): the
 * pipeline adapts the share step by step -- towards the GPU while a step waits for host work after its dense flow is done, back towards the host while
 * no step waits (the smallest GPU share the host keeps up with).  Environment SIND_GROW_GPU=0..4 fixes it at create. */
int sind_pipe_set_grow_share(sind_pipe* p, int quarters);
int sind_pipe_get_grow_share(sind_pipe* p, int* quarters);
/* How many groups of streams run their batched k-means rounds (reference DynaDetect.cc:315-420) as independent chains at the moment: 1..4 (at most streams / 8)
 * chosen by the same controller (one more while steps wait for the host although every region grow already runs on the GPU).  Results do not depend on it. */
int sind_pipe_set_kmeans_groups(sind_pipe* p, int groups);      /* 1 .. min(4, streams / 8), or -1 = adaptive (default); takes effect with the next step */
int sind_pipe_get_kmeans_groups(sind_pipe* p, int* groups);
/* Flow-mask stage of the tails (DynaDetect.cc:1252-1367: residual against the homography, histogram, Otsu / Triangle thresholds, both masks) batched per round:
 * where a step runs as rounds whose k-means waits for whole tails (more streams than pool workers), the homographies of one frame of every stream of a group are
 * computed on the pool while the batched k-means runs, and the stage's kernels run once for the group instead of once per frame; the masks come back bit-packed.
 * Same results.  on = 0 runs the stage per frame everywhere (default 1).  Setting the switch resets the counter: frames_batched = frames whose masks came from a
 * batch since then.  Not while a submitted step is pending. */
int sind_pipe_set_flow_mask_batch(sind_pipe* p, int on);
int sind_pipe_get_flow_mask_batch(sind_pipe* p, int* on, long long* frames_batched);
/* Region-adjacency (RAG) stage of SegAndMerge in the tails (the 7 x 7 dilation of every piece and the overlap / connection / histogram counts over the pieces' bit planes)
 * batched in the same rounds: a frame's tail runs up to the packed planes, joins the round's batch of its k-means group, and continues from the returned counters; a
 * chunk of frames costs one plane upload, one record upload, two launches and one copy back instead of that per frame.  Same results (integer counts).  on = 0 runs the
 * stage per frame everywhere (default 1).  Setting the switch resets the counters: frames_batched = frames of batched rounds that did not take the per-frame stage
 * (a frame without pieces needs no counts and is one of them), frames_fallback = frames the slab had no room for, which took the per-frame stage.
 * chunk_frames: frames per set of launches (< 1: a whole group; default 32).  slab_planes_per_frame: the page-locked and device slabs hold that many input planes (two
 * per piece) times the frames of a group (default 64; < 0: keep).  Not while a submitted step is pending. */
int sind_pipe_set_rag_batch(sind_pipe* p, int on);
int sind_pipe_get_rag_batch(sind_pipe* p, int* on, long long* frames_batched, long long* frames_fallback);
int sind_pipe_set_rag_batch_chunk(sind_pipe* p, int chunk_frames, int slab_planes_per_frame);

/* ------------------------------------------------------------------------------------------------------------
 * Frame post-ORB steps: what the reference's RGB-D Frame constructor does with the extractor's output
 * (ORB_SLAM2/src/Frame.cc:143-170) for B frames at once:
 *   UndistortKeyPoints()           src/Frame.cc:477-509  -> un_xy   [B][cap][2]  mvKeysUn[i].pt  (identity when k1 == 0)
 *   ComputeStereoFromRGBD(imDepth) src/Frame.cc:714-735  -> depth_out / u_right [B][cap]  mvDepth / mvuRight (-1 when d <= 0)
 *   ComputeImageBounds(imGray)     src/Frame.cc:511-541  -> bounds4 = {mnMinX, mnMaxX, mnMinY, mnMaxY}
 *   AssignFeaturesToGrid()         src/Frame.cc:283-299  -> cell [B][cap] = x * 48 + y (-1: PosInGrid false) and mGrid as CSR:
 *                                                           grid_start [B][3073], grid_idx [B][cap] (push_back order)
 * calib: mK, mDistCoef (k1 k2 p1 p2 k3), Camera.bf, depth_map_factor = 1 / DepthMapFactor (src/Tracking.cc:262-263 converts the
 * raw u16 depth with it).  kps [B][cap] / nkp [B]: the extractor's output (host).  depth: raw u16 [B][height][width], host or
 * device pointer (depth_on_device).  Output pointers are host and may be NULL.
 */
typedef struct sind_frame sind_frame;
typedef struct sind_frame_calib { float fx, fy, cx, cy, k1, k2, p1, p2, k3, bf, depth_map_factor; } sind_frame_calib;
int sind_frame_create(const sind_frame_calib* calib, int width, int height, int max_batch, int cap, int device, sind_frame** out);
int sind_frame_destroy(sind_frame* f);
int sind_frame_post_orb(sind_frame* f, const sind_keypoint* kps, const int* nkp, int B, const uint16_t* depth, int depth_on_device,
                        float* un_xy, float* u_right, float* depth_out, int* cell, int* grid_start, int* grid_idx, float* bounds4);

/* ------------------------------------------------------------------------------------------------------------
 * Projection matcher.  Replaces, for B (CurrentFrame, LastFrame) pairs at once,
 *   int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool bMono)   src/ORBmatcher.cc:1328-1470
 * including Frame::GetFeaturesInArea (src/Frame.cc:398-451), ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1647-1665), the
 * rotation histogram and ComputeThreeMaxima (:1601-1642).  The Frame / MapPoint object graph is passed as flat arrays:
 *   last frame, per keypoint i:  x3Dw = pMP->GetWorldPos(), last_valid = (pMP && !mvbOutlier[i]), last_has_obs = pMP->Observations() > 0,
 *                                last_octave = mvKeys[i].octave, last_angle = mvKeysUn[i].angle, last_desc = pMP->GetDescriptor() (32 B)
 *   current frame, per keypoint: cur_un_xy / cur_octave / cur_angle = mvKeysUn, cur_u_right = mvuRight, cur_desc = mDescriptors rows,
 *                                grid_start / grid_idx = mGrid (as sind_frame_post_orb returns it), cur_taken = mvpMapPoints[i2] &&
 *                                Observations() > 0 on entry (NULL = all free, the TrackWithMotionModel case src/Tracking.cc:914)
 * Output: match_of_cur[i2] = index i of the last-frame keypoint whose MapPoint the reference stores in
 * CurrentFrame.mvpMapPoints[i2] (-1: none or removed by the orientation check); *nmatches = the function's return value.
 * config: fx fy cx cy bf of the current frame, bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY}, scale_factors = mvScaleFactors.
 * mCheckOrientation is the matcher's constructor flag (src/ORBmatcher.cc:41); nnratio is not used by this overload.
 */
typedef struct sind_match sind_match;
typedef struct sind_match_config { float fx, fy, cx, cy, bf; float bounds[4]; float scale_factors[16]; int nlevels, cap_last, cap_cur, max_batch, device; } sind_match_config;
typedef struct sind_match_pair {
    const float* Tcw_cur; const float* Tcw_last;                     /* 4x4 row-major poses (rows 0..2 are read) */
    int n_last; const float* x3Dw; const uint8_t* last_valid; const uint8_t* last_has_obs; const int* last_octave; const float* last_angle; const uint8_t* last_desc;
    int n_cur; const float* cur_un_xy; const int* cur_octave; const float* cur_angle; const float* cur_u_right; const uint8_t* cur_desc;
    const int* grid_start; const int* grid_idx; const uint8_t* cur_taken;
    int* match_of_cur; int* nmatches;                                /* outputs (host) */
} sind_match_pair;
int sind_match_create(const sind_match_config* cfg, sind_match** out);
int sind_match_destroy(sind_match* m);
int sind_match_by_projection(sind_match* m, const sind_match_pair* pairs, int B, float th, int mono, int check_orientation);
int sind_match_last_rounds(sind_match* m);      /* resolution rounds the last call needed (see csrc/match_kernels.hip) */

/* Local-map search.  Replaces, for B frames at once, the body of Tracking::SearchLocalPoints from its second loop on (src/Tracking.cc:1203-1229):
 *   bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit)                                     src/Frame.cc:340-396
 *   int MapPoint::PredictScale(const float& currentDist, Frame* pF)                                   src/MapPoint.cc:402-418
 *   int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th)  src/ORBmatcher.cc:45-129, RadiusByViewingCos :131-137
 * The frame's intrinsics, bounds and scale factors are the handle's (sind_match_config); the capacity for map points per frame is set by
 * sind_match_reserve_map_points (once, or again to grow), which must precede the first sind_match_local_map (SIND_E_STATE otherwise).
 *   Tcw = F.mTcw (4x4 row-major, rows 0..2 are read; mRcw, mtcw and mOw are derived from it as Frame::UpdatePoseMatrices does)
 *   map points, per entry i of mvpLocalMapPoints:  x3Dw = pMP->GetWorldPos(), normal = pMP->GetNormal(), max_dist / min_dist = the members mfMaxDistance /
 *       mfMinDistance (not the Get...Invariance() values), flags bit0 = !pMP->isBad() && pMP->mnLastFrameSeen != F.mnId, bit1 = pMP->Observations() > 0,
 *       desc = pMP->GetDescriptor() (32 B)
 *   current frame, per keypoint: cur_un_xy / cur_octave = mvKeysUn, cur_u_right = mvuRight, cur_desc = mDescriptors rows, grid_start / grid_idx = mGrid (as
 *       sind_frame_post_orb returns it), cur_taken = mvpMapPoints[idx] && mvpMapPoints[idx]->Observations() > 0 on entry (NULL = all free)
 * Outputs (host): in_view = pMP->mbTrackInView, proj_xyr = {mTrackProjX, mTrackProjY, mTrackProjXR} (3 floats per point), level = mnTrackScaleLevel,
 * view_cos = mTrackViewCos (all zero where in_view is 0), *n_to_match = nToMatch; each of the five may be NULL.  match_of_cur[idx] = index i of the map
 * point the reference leaves in F.mvpMapPoints[idx] (-1: the search wrote nothing there), *nmatches = the function's return value (it counts every
 * assignment, overwritten ones included).  The caller still does IncreaseVisible() for the points in view and the mnLastFrameSeen bookkeeping.
 * th: 1 / 3 / 5 of the tracker; nnratio: ORBmatcher::mfNNratio (0.8 there); viewing_cos_limit: 0.5 there.
 * std::log in PredictScale and in Frame::mfLogScaleFactor is evaluated as the FP64 logarithm rounded to FP32 (see csrc/match_local.hip).
 * Errors: a frame over capacity -> SIND_E_CAPACITY, a NULL array with a non-zero count or a malformed grid -> SIND_E_ARG; nothing is launched.
 */
int sind_match_reserve_map_points(sind_match* m, int cap_points);
typedef struct sind_match_local {
    const float* Tcw;
    int n_points; const float* x3Dw; const float* normal; const float* max_dist; const float* min_dist; const uint8_t* flags; const uint8_t* desc;
    int n_cur; const float* cur_un_xy; const int* cur_octave; const float* cur_u_right; const uint8_t* cur_desc;
    const int* grid_start; const int* grid_idx; const uint8_t* cur_taken;
    uint8_t* in_view; float* proj_xyr; int* level; float* view_cos; int* n_to_match;      /* outputs (host), may be NULL */
    int* match_of_cur; int* nmatches;                                                     /* outputs (host) */
} sind_match_local;
int sind_match_local_map(sind_match* m, const sind_match_local* frames, int B, float th, float nnratio, float viewing_cos_limit);

/* Relocalisation search.  Replaces, for B (CurrentFrame, KeyFrame) pairs at once,
 *   int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th, const int ORBdist)
 *                                                                                                      src/ORBmatcher.cc:1472-1599
 * (Tracking::Relocalization calls it with th 10 / ORBdist 100 and th 3 / ORBdist 64).  At most cap_last key-frame slots and cap_cur keypoints per pair.
 *   Tcw = CurrentFrame.mTcw
 *   key frame, per slot i of pKF->GetMapPointMatches():  valid = pMP && !pMP->isBad() && !sAlreadyFound.count(pMP), x3Dw = pMP->GetWorldPos(),
 *       max_dist / min_dist = mfMaxDistance / mfMinDistance, kf_angle = pKF->mvKeysUn[i].angle, desc = pMP->GetDescriptor() (32 B)
 *   current frame, per keypoint: cur_un_xy / cur_octave / cur_angle = mvKeysUn, cur_desc = mDescriptors rows, grid_start / grid_idx = mGrid,
 *       cur_taken = CurrentFrame.mvpMapPoints[i2] != NULL on entry (NULL = all free)
 * Output: match_of_cur[i2] = slot i whose MapPoint the reference stores in CurrentFrame.mvpMapPoints[i2] (-1: none or removed by the orientation check);
 * *nmatches = the function's return value.  check_orientation = ORBmatcher::mbCheckOrientation.  Errors as above.
 */
typedef struct sind_match_reloc {
    const float* Tcw;
    int n_points; const float* x3Dw; const float* max_dist; const float* min_dist; const uint8_t* valid; const float* kf_angle; const uint8_t* desc;
    int n_cur; const float* cur_un_xy; const int* cur_octave; const float* cur_angle; const uint8_t* cur_desc;
    const int* grid_start; const int* grid_idx; const uint8_t* cur_taken;
    int* match_of_cur; int* nmatches;                                                     /* outputs (host) */
} sind_match_reloc;
int sind_match_by_projection_kf(sind_match* m, const sind_match_reloc* frames, int B, float th, int orb_dist, int check_orientation);

/* Vocabulary transform: the feature-vector half of Frame::ComputeBoW / KeyFrame::ComputeBoW, for B frames at once.  Replaces
 *   void TemplatedVocabulary::transform(features, BowVector& v, FeatureVector& fv, int levelsup)        Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194
 *   void TemplatedVocabulary::transform(feature, WordId&, WordValue&, NodeId* nid, int levelsup)        :1218-1259, with FORB::distance (Hamming)
 * sind_voc holds one vocabulary tree on the device; the caller flattens DBoW2's object graph once (sind_voc_tree):
 *   n_nodes = m_nodes.size() (node 0 is the root), levels = m_L, child_start / child = CSR over m_nodes[i].children in the vector's own order,
 *   desc = m_nodes[i].descriptor (32 B per node, row 0 is not read), word_id = m_nodes[i].word_id for a leaf and -1 for an inner node,
 *   weight = m_nodes[i].weight (read for leaves only).
 * sind_voc_create checks that this is a tree rooted at node 0 with at least one child under the root (indices in range, every other node the child of exactly
 * one node and reachable from the root, every childless node with word_id >= 0) and returns SIND_E_ARG otherwise.
 * sind_voc_transform, per descriptor: the descent from the root takes at every level the child of smallest Hamming distance, the first one on equal distance,
 * and stops at a childless node.  word_id = that leaf's word.  node_id = the node the path passed at level (levels - levelsup), the reference's nid
 * (ORB-SLAM2 passes levelsup = 4); 0 if levels - levelsup <= 0; the leaf's own id if the path ends above that level (the reference leaves nid uninitialised
 * there); -1 if the word is stopped, !(weight > 0): such a feature is not in mFeatVec (:1157-1161).  DBoW2 fills mFeatVec in feature order
 * (FeatureVector.cpp:31-45), so node_id per keypoint determines it: nodes ascend, indices ascend inside a node.  The BowVector (word weights, normalisation) is
 * left to the caller, who gets word_id for it, or comes from sind_voc_transform_bow below.
 *   desc[b] = n[b] x 32 bytes (host); node_id[b], word_id[b] = n[b] ints (host); node_id, word_id and their entries may be NULL.
 * Errors: n[b] > cap or B > max_batch -> SIND_E_CAPACITY, a NULL desc[b] with n[b] > 0 -> SIND_E_ARG; nothing is launched, the outputs are untouched.
 */
typedef struct sind_voc sind_voc;
typedef struct sind_voc_tree {
    int n_nodes, levels;
    const int* child_start;       /* [n_nodes + 1] */
    const int* child;             /* [n_nodes - 1] */
    const uint8_t* desc;          /* [n_nodes][32] */
    const int* word_id;           /* [n_nodes] */
    const double* weight;         /* [n_nodes] */
} sind_voc_tree;
int sind_voc_create(const sind_voc_tree* tree, int cap, int max_batch, int device, sind_voc** out);
int sind_voc_destroy(sind_voc* v);
int sind_voc_transform(sind_voc* v, const uint8_t* const* desc, const int* n, int B, int levelsup, int* const* node_id, int* const* word_id);

/* The whole of ComputeBoW: sind_voc_transform and the BowVector, for B frames at once, without a host step between the descent and the vector.  Adds
 *   the BowVector half of TemplatedVocabulary::transform(features, v, fv, levelsup)                      Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194
 *   void BowVector::addWeight(WordId id, WordValue v)                                                    Thirdparty/DBoW2/DBoW2/BowVector.cpp:34-46
 *   void BowVector::normalize(LNorm norm_type)                                                           :62-84
 * for TF_IDF weighting and L1_NORM scoring, the ORB vocabulary's; no other mode is implemented (TF would be the same with weights of 1; IDF / BINARY use
 * addIfNotExist, and the L2 norm and the "divide by size" of a scoring that does not normalise are absent).
 * node_id / word_id are sind_voc_transform's, bit for bit.  bow_word[b] / bow_value[b] = the std::map<WordId, WordValue> of frame b in its iteration order:
 * n_words[b] <= n[b] entries, word ids strictly ascending; the caller gives room for n[b] of each, the entries past n_words[b] are left alone.
 * The values are the reference's FP64 operations in the reference's order:
 *   value of a word = the weight of the leaf, added once per feature that fell on the word, in feature order, starting from the first weight:
 *       w, w + w, (w + w) + w, ...  -- not count * w; a stopped word, !(w > 0), is absent (:1157);
 *   norm = the sum of fabs(value) over ascending word id, left to right;  if norm > 0 every value becomes value / norm (IEEE division);
 *   a frame without a word that counts has n_words[b] = 0.
 * The weights stay on the device as the FP64 given to sind_voc_create.  A frame holds at most min(cap, 4096) descriptors here (one workgroup sorts a frame's
 * words in LDS, as for the two searches by vocabulary node).
 * Errors as for sind_voc_transform (n[b] over that limit or B > max_batch -> SIND_E_CAPACITY; a NULL desc[b], bow_word[b] or bow_value[b] with n[b] > 0, or a
 * NULL bow_word, bow_value or n_words -> SIND_E_ARG): nothing is launched, the outputs are untouched.
 */
int sind_voc_transform_bow(sind_voc* v, const uint8_t* const* desc, const int* n, int B, int levelsup, int* const* node_id, int* const* word_id,
                           int* const* bow_word, double* const* bow_value, int* n_words /* [B] */);

/* Key-frame database: the scoring of KeyFrameDatabase on the device.  Replaces the inverted file and the scores of
 *   void KeyFrameDatabase::add(KeyFrame*), ::erase(KeyFrame*), ::clear()                                 src/KeyFrameDatabase.cc:40-73
 *   vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore)              :76-197
 *   vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F)                         :199-309
 *   double L1Scoring::score(const BowVector& v1, const BowVector& v2)                                    Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
 * and serves mpORBVocabulary->score against the connected key frames in LoopClosing::DetectLoop (src/LoopClosing.cc:124-141): minScore is the smallest
 * `score` among the connected key frames' slots.
 * A slot is the caller's index for a key frame (0 .. cap_slots - 1).  The BowVectors live on the device, cap_words per slot.
 *   add     stores a BowVector (word ids >= 0, strictly ascending, as sind_voc_transform_bow returns them) in a dead slot and gives the slot the next value of a
 *           sequence counter (sind_bowdb_sequence; -1 for a dead slot).  The reference keeps one list<KeyFrame*> per word in push_back order and erase
 *           keeps the order of the others, so every list is ordered by that counter.
 *   erase   makes the slot dead; erasing a dead slot does nothing, as in the reference.  clear makes every slot dead; the counter runs on.
 *   query   Q query vectors at once.  For every live slot:  common = the number of words both vectors hold = mnLoopWords / mnRelocWords;
 *           first_word = the smallest common word, -1 if none;  score = (float)(-sum / 2.0), sum = the FP64 sum over the common words in ascending order of
 *           fabs(vi - wi) - fabs(vi) - fabs(wi) (vi the query's value, wi the slot's), evaluated left to right without contraction, added one term after
 *           another: the float the reference stores in mLoopScore / mRelocScore.  Dead slots get 0, -1 and 0.0f.
 * The reference scores only key frames with more than minCommonWords common words; here every live slot is scored and the caller filters: the values of
 * the ones the reference scores are the reference's.  The list and graph logic that follows is order-dependent and stays with the caller (INTEGRATION.md
 * gives it in C++, sindslam_amd/keyframe_db.py in Python): lKFsSharingWords is the live slots with common > 0 (without the connected key frames for the
 * loop version) ordered by (first_word, sequence).
 * One point is a definition, not a reproduction: DetectRelocalizationCandidates adds pKF2->mRelocScore for any neighbour that shares a word with the frame,
 * also one that was not scored in this query (:273-276), and the reference never initialises that member (src/KeyFrame.cc:35).  The tails given with this
 * library keep a per-slot reloc_score that is 0.0f at add and overwritten only when the slot is scored.
 * Errors: a slot outside [0, cap_slots), a NULL array with a non-zero count, a NULL output, words that do not ascend strictly -> SIND_E_ARG; more than
 * cap_words words or Q > max_queries -> SIND_E_CAPACITY; add on a live slot -> SIND_E_STATE.  Nothing is launched, the database and the outputs are untouched.
 */
typedef struct sind_bowdb sind_bowdb;
int sind_bowdb_create(int cap_slots, int cap_words, int max_queries, int device, sind_bowdb** out);
int sind_bowdb_destroy(sind_bowdb* db);
int sind_bowdb_add(sind_bowdb* db, int slot, const int* word, const double* value, int n);
int sind_bowdb_erase(sind_bowdb* db, int slot);
int sind_bowdb_clear(sind_bowdb* db);
long long sind_bowdb_sequence(const sind_bowdb* db, int slot);
typedef struct sind_bowdb_query_item {
    int n; const int* word; const double* value;                                          /* the query's BowVector */
    int* common; int* first_word; float* score;                                           /* outputs (host), [cap_slots] each */
} sind_bowdb_query_item;
int sind_bowdb_query(sind_bowdb* db, const sind_bowdb_query_item* q, int Q);

/* Search by vocabulary node.  Replaces, for B (KeyFrame, Frame) pairs at once,
 *   int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)          src/ORBmatcher.cc:159-288
 * (Tracking::TrackReferenceKeyFrame; Tracking::Relocalization runs it once per candidate key frame: one frame against many key frames is one call).
 * Runs on the sind_match handle: at most min(cap_last, 4096) key-frame keypoints and min(cap_cur, 4096) frame keypoints per pair.
 *   key frame, per keypoint i:  kf_node = node id of pKF->mFeatVec as sind_voc_transform returns it (-1: not in the feature vector),
 *       kf_valid = pMP && !pMP->isBad() for pMP = pKF->GetMapPointMatches()[i], kf_angle = pKF->mvKeysUn[i].angle,
 *       kf_desc = row i of pKF->mDescriptors (the key frame's own descriptor, not the map point's)
 *   frame, per keypoint:  cur_node = node id of F.mFeatVec, cur_angle = F.mvKeys[i].angle, cur_desc = row i of F.mDescriptors
 * Output: match_of_cur[iF] = index i of the key-frame keypoint whose MapPoint the reference leaves in vpMapPointMatches[iF] (-1: none, or removed by the
 * orientation check); *nmatches = the function's return value.  nnratio = ORBmatcher::mfNNratio (0.7 in TrackReferenceKeyFrame, 0.75 in Relocalization),
 * check_orientation = mbCheckOrientation.  TH_LOW = 50, the ratio test in FP32, 30 histogram bins: the reference's.
 * The result is that of the reference's order (nodes ascending, key-frame entries ascending inside a node, frame keypoints already matched skipped).
 * Errors: a pair over capacity -> SIND_E_CAPACITY, a NULL array with a non-zero count or a node id below -1 -> SIND_E_ARG; nothing is launched and the
 * outputs are untouched.  A count of 0 is valid and gives *nmatches = 0.
 */
typedef struct sind_match_bow {
    int n_kf;  const int* kf_node;  const uint8_t* kf_valid;  const float* kf_angle;  const uint8_t* kf_desc;
    int n_cur; const int* cur_node; const float* cur_angle;   const uint8_t* cur_desc;
    int* match_of_cur; int* nmatches;                                                     /* outputs (host) */
} sind_match_bow;
int sind_match_by_bow(sind_match* m, const sind_match_bow* pairs, int B, float nnratio, int check_orientation);

/* Search by vocabulary node between two key frames.  Replaces, for B (pKF1, pKF2) pairs at once,
 *   int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)         src/ORBmatcher.cc:522-655
 * (LoopClosing::ComputeSim3, src/LoopClosing.cc:265, once per loop candidate with ORBmatcher(0.75, true): the current key frame against all candidates is one
 * call, and the pairs may share side 1's arrays).  Capacities as for sind_match_by_bow: side 1 at most min(cap_last, 4096), side 2 at most min(cap_cur, 4096).
 *   per side s (1, 2) and keypoint i:  nodes = node id of pKFs->mFeatVec (-1: not in it), valids = pMP && !pMP->isBad() for pMP = pKFs->GetMapPointMatches()[i],
 *       angles = pKFs->mvKeysUn[i].angle, descs = row i of pKFs->mDescriptors
 * Output: match12[idx1] = idx2 of the map point the reference leaves in vpMatches12[idx1] (-1: none, or removed by the orientation check); *nmatches = the
 * function's return value.  What differs from sind_match_by_bow: both sides carry validity, a keypoint of side 2 is closed once matched (vbMatched2), the
 * result and the rotation histogram are indexed by idx1, both angles are the undistorted keypoints', and the bound is bestDist1 < TH_LOW (50), strict.
 * Errors as for sind_match_by_bow.
 */
typedef struct sind_match_bow_kf {
    int n1; const int* node1; const uint8_t* valid1; const float* angle1; const uint8_t* desc1;
    int n2; const int* node2; const uint8_t* valid2; const float* angle2; const uint8_t* desc2;
    int* match12; int* nmatches;                                                          /* outputs (host): match12[idx1] = idx2 or -1 */
} sind_match_bow_kf;
int sind_match_by_bow_kf(sind_match* m, const sind_match_bow_kf* pairs, int B, float nnratio, int check_orientation);

/* Search for triangulation.  Replaces, for B (pKF1, pKF2) pairs at once (LocalMapping::CreateNewMapPoints, one key frame against its neighbours),
 *   int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vector<pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo)
 *                                                                                                      src/ORBmatcher.cc:657-823
 *   bool ORBmatcher::CheckDistEpipolarLine(kp1, kp2, F12, pKF2)                                        :140-157
 * fx fy cx cy and scale_factors (mvScaleFactors; mvLevelSigma2[l] = scale[l] * scale[l] in FP32) are the handle's.  Capacities as for sind_match_by_bow
 * (pKF1: cap_last, pKF2: cap_cur).
 *   Tcw2 = pKF2's pose (4x4 row-major, rows 0..2 are read: GetRotation(), GetTranslation()), Cw1 = pKF1->GetCameraCenter() (3), F12 (3x3 row-major)
 *   per keypoint of pKF1:  node1 = node id of mFeatVec, has_mp1 = pKF1->GetMapPoint(idx1) != NULL, un_xy1 / angle1 = mvKeysUn, u_right1 = mvuRight,
 *       desc1 = mDescriptors rows
 *   per keypoint of pKF2:  node2, has_mp2, un_xy2 / octave2 / angle2 = mvKeysUn, u_right2, desc2 likewise
 * Output: match12[idx1] = vMatches12[idx1] after the orientation check (idx2 or -1), from which vMatchedPairs is the list of (idx1, match12[idx1]) with
 * match12[idx1] >= 0 in ascending idx1; *nmatches = the function's return value.  only_stereo = bOnlyStereo, check_orientation = mbCheckOrientation.
 * The epipole, the epipolar line and its distance are FP32 in the reference's order of operations; the last comparison is in FP64 (csrc/match_bow.hip).
 * Errors as for sind_match_by_bow, and an octave2 outside [0, nlevels) -> SIND_E_ARG.
 */
typedef struct sind_match_tri {
    const float* Tcw2; const float* Cw1; const float* F12;
    int n1; const int* node1; const uint8_t* has_mp1; const float* un_xy1; const float* angle1; const float* u_right1; const uint8_t* desc1;
    int n2; const int* node2; const uint8_t* has_mp2; const float* un_xy2; const int* octave2; const float* angle2; const float* u_right2; const uint8_t* desc2;
    int* match12; int* nmatches;                                                          /* outputs (host): match12[idx1] = idx2 or -1 */
} sind_match_tri;
int sind_match_for_triangulation(sind_match* m, const sind_match_tri* pairs, int B, int only_stereo, int check_orientation);

/* Projections of map points into a key frame: the local mapper's Fuse and the three searches of the loop closer.  All run on the sind_match handle; intrinsics,
 * bounds, scale factors and nlevels are the handle's, map points per item are limited by sind_match_reserve_map_points (SIND_E_STATE before it) and key-frame
 * keypoints by cap_cur.  A key frame keeps mnMinX .. mnMaxY as int (include/KeyFrame.h:185-188): the handle's bounds are truncated toward zero for
 * KeyFrame::IsInImage and the window, and mfGridElementWidthInv / HeightInv stay those of the float bounds, as the KeyFrame constructor copies them.
 * Common to the three calls:
 *   KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608), KeyFrame::IsInImage (:610-613: the upper bounds are strict),
 *   MapPoint::PredictScale(dist, KeyFrame*) (src/MapPoint.cc:385-400; std::log as for sind_match_local_map), ORBmatcher::DescriptorDistance.
 *   map points, per entry i of the list:  x3Dw = pMP->GetWorldPos(), normal = pMP->GetNormal(), max_dist / min_dist = the members mfMaxDistance / mfMinDistance
 *       (the 1.2f / 0.8f of Get...DistanceInvariance() are applied inside), desc = pMP->GetDescriptor() (32 B), valid: see each call
 *   key frame, per keypoint:  kf_un_xy / kf_octave = mvKeysUn, kf_desc = mDescriptors rows, grid_start / grid_idx = mGrid in the sind_frame_post_orb layout
 * Errors: an item over capacity -> SIND_E_CAPACITY; a NULL array with a non-zero count, a malformed grid or a kf_octave outside [0, nlevels) -> SIND_E_ARG;
 * nothing is launched and the outputs are untouched.  A count of 0 is valid.  The small-matrix algebra (Scw decomposition, sR12, sR21, t21) is done on the host
 * once per item, rounded as csrc/match_local.hip (5)-(7) defines it.
 *
 * sind_match_fuse.  Replaces, for B (key frame, point list) items at once, the search of
 *   int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th)               src/ORBmatcher.cc:825-949   (sim3 = 0)
 *   int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint)   :977-1079   (sim3 = 1)
 * (LocalMapping::SearchInNeighbors, th 3; LoopClosing::SearchAndFuse, th 4).
 *   Tcw: sim3 = 0: pKF->GetPose(); sim3 = 1: Scw, decomposed as :986-990 (4x4 row-major, rows 0..2 are read)
 *   valid: sim3 = 0: pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF); sim3 = 1: !pMP->isBad() && !spAlreadyFound.count(pMP)
 *   kf_u_right = mvuRight: read for sim3 = 0 only (the chi-square test :914-938, mvInvLevelSigma2[l] = 1.0f / (scale[l] * scale[l])); may be NULL for sim3 = 1
 * Outputs, per point: best_idx[i] = bestIdx if bestDist <= TH_LOW (50), else -1; best_dist[i] = bestDist where best_idx[i] >= 0, else -1;
 * *nfused = number of best_idx[i] >= 0 = the function's return value for the inputs as given.
 * The tail on the object graph (:952-971, :1082-1096: GetMapPoint(bestIdx), Replace, AddObservation, AddMapPoint, vpReplacePoint[iMP]) stays with the caller,
 * who replays it in point order over the entries with best_idx[i] >= 0.  For sim3 = 0 the caller re-tests isBad() || IsInKeyFrame(pKF) before applying entry i
 * and skips it, uncounted, if true.  This replay reproduces the reference: the search of point i reads only point i's own position, normal, distances and
 * descriptor and the key frame's immutable arrays (mvKeysUn, mvuRight, mDescriptors, mGrid), and within one call an earlier iteration changes a point's own data
 * only (a) for a point that was already in pKF (Replace on pMPinKF: such a point is filtered by `valid`, and by the re-test if it got into pKF during the call),
 * or (b) for a point that has itself been processed (Replace makes it bad after its own iteration; AddObservation does not touch what the search reads).  The
 * survivor of a Replace gets a new descriptor only through ComputeDistinctiveDescriptors, and the survivor is either pMPinKF (case a) or pMP, already
 * processed (case b).  A repeated list entry was either added to pKF (IsInKeyFrame) or replaced (isBad) by its first occurrence: the re-test catches both.
 * For sim3 = 1 nothing in the loop changes what `valid` is made of: spAlreadyFound is a snapshot in the reference (:993) and the loop sets no bad flag.
 * NOT exact: batching one point list over several target key frames (LocalMapping.cc:485-490) searches every key frame against the list as it was on entry,
 * whereas the reference lets key frame k's Replace calls change the list for key frame k+1 (a bad flag, a recomputed descriptor).  Exactness needs one item
 * per call with refreshed inputs.
 */
typedef struct sind_match_fuse_item {
    const float* Tcw;                                                                     /* pose (sim3 = 0) or Scw (sim3 = 1) */
    int n_points; const float* x3Dw; const float* normal; const float* max_dist; const float* min_dist; const uint8_t* valid; const uint8_t* desc;
    int n_kf; const float* kf_un_xy; const int* kf_octave; const float* kf_u_right; const uint8_t* kf_desc; const int* grid_start; const int* grid_idx;
    int* best_idx; int* best_dist; int* nfused;                                           /* outputs (host): [n_points], [n_points], [1] */
} sind_match_fuse_item;
int sind_match_fuse(sind_match* m, const sind_match_fuse_item* items, int B, float th, int sim3);

/* sind_match_by_projection_sim3.  Replaces, for B items at once,
 *   int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th)   src/ORBmatcher.cc:290-403
 * (LoopClosing::ComputeSim3, th 10).  Points as above with valid = !pMP->isBad() && !spAlreadyFound.count(pMP); the key frame as above without kf_u_right, and
 * kf_taken[idx] = vpMatched[idx] != NULL on entry (NULL = none).  th is the reference's int: the radius is (float)th * mvScaleFactors[level].
 * Output: match_of_kf[idx] = index i of the point the reference writes to vpMatched[idx] (-1: untouched); *nmatches = the function's return value.
 * The reference's order is kept: a keypoint matched by point j is skipped by every later point, before its distance is computed (:375).
 * sind_match_last_rounds reports the resolution rounds this took.
 */
typedef struct sind_match_proj_sim3 {
    const float* Scw;
    int n_points; const float* x3Dw; const float* normal; const float* max_dist; const float* min_dist; const uint8_t* valid; const uint8_t* desc;
    int n_kf; const float* kf_un_xy; const int* kf_octave; const uint8_t* kf_desc; const int* grid_start; const int* grid_idx; const uint8_t* kf_taken;
    int* match_of_kf; int* nmatches;                                                      /* outputs (host): [n_kf], [1] */
} sind_match_proj_sim3;
int sind_match_by_projection_sim3(sind_match* m, const sind_match_proj_sim3* items, int B, int th);

/* sind_match_by_sim3.  Replaces, for B (pKF1, pKF2) pairs at once,
 *   int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12, const float th)
 *                                                                                                      src/ORBmatcher.cc:1102-1326
 * (LoopClosing::ComputeSim3, th 7.5).  Each side holds at most min(cap_last, cap_cur) slots; sind_match_reserve_map_points is not needed.
 *   T1w, T2w = poses of pKF1 / pKF2 (4x4 row-major, rows 0..2 are read), s12, R12 (3x3 row-major), t12 (3); sR12, sR21 and t21 are formed as :1119-1121
 *   per side s (1, 2) and slot i of pKFs->GetMapPointMatches():  valid = pMP && !pMP->isBad() && !vbAlreadyMatcheds[i] (the caller builds vbAlreadyMatched1/2 as
 *       :1132-1142), x3Dw / max_dist / min_dist / mp_desc = pMP->GetWorldPos(), mfMaxDistance, mfMinDistance, pMP->GetDescriptor() of the map point in that slot;
 *       the slot's own keypoint: un_xy / octave = mvKeysUn[i], kf_desc = row i of mDescriptors; grid_start / grid_idx = the side's mGrid
 * Output: match12[i1] = idx2 where vnMatch1[i1] == idx2 && vnMatch2[idx2] == i1, else -1: the slots whose vpMatches12[i1] the reference sets to
 * vpMapPoints2[idx2]; *nfound = the function's return value.  TH_HIGH = 100; no viewing-angle test; the distance is the norm of the camera-frame vector.
 */
typedef struct sind_match_sim3_side {
    int n; const uint8_t* valid; const float* x3Dw; const float* max_dist; const float* min_dist; const uint8_t* mp_desc;
    const float* un_xy; const int* octave; const uint8_t* kf_desc; const int* grid_start; const int* grid_idx;
} sind_match_sim3_side;
typedef struct sind_match_sim3_pair {
    const float* T1w; const float* T2w; float s12; const float* R12; const float* t12;
    sind_match_sim3_side side1, side2;
    int* match12; int* nfound;                                                            /* outputs (host): [side1.n], [1] */
} sind_match_sim3_pair;
int sind_match_by_sim3(sind_match* m, const sind_match_sim3_pair* pairs, int B, float th);

/* sind_match_sim3_ransac.  Replaces, for B loop candidates at once and for all of their RANSAC iterations, the arithmetic of
 *   Sim3Solver::Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale)            src/Sim3Solver.cc:37-112  (from :84 on: the per-correspondence values)
 *   void Sim3Solver::ComputeSim3(cv::Mat& P1, cv::Mat& P2)                :226-337, ComputeCentroid :215-224
 *   void Sim3Solver::CheckInliers()                                       :340-364, Project :382-403, FromCameraToImage :405-423
 * (LoopClosing::ComputeSim3, src/LoopClosing.cc:274-301: the solver that turns the matches of sind_match_by_bow_kf into the s12, R12, t12 that
 * sind_match_by_sim3 takes).  In Sim3Solver::iterate (:140-207) the sample of an iteration depends only on the random stream and on N, so the caller draws
 * every triple beforehand, this call evaluates all of them, and iterate's bookkeeping (mnBestInliers, the early return, bNoMore, five iterations per candidate
 * in turn) is a replay over `count` (INTEGRATION.md gives it in C++, sindslam_amd/sim3.py in Python).  Runs on the sind_match handle; fx fy cx cy are the
 * handle's (the reference's mK1 and mK2 are the same matrix in an RGB-D run).
 *   T1w, T2w = pKF1->GetPose(), pKF2->GetPose() (GetRotation / GetTranslation are their blocks)
 *   per correspondence, i.e. per i1 that passes the tests of :64-79, in ascending i1 (the caller keeps mvnIndices1):
 *       x3Dw1 = pMP1->GetWorldPos(), x3Dw2 = pMP2->GetWorldPos(), sigma2_1 = pKF1->mvLevelSigma2[kp1.octave], sigma2_2 = pKF2->mvLevelSigma2[kp2.octave]
 *       (finite, >= 0).  The bound is (size_t)(9.210 * sigma2) as include/Sim3Solver.h:78-79 declares mvnMaxError1/2: an integer.
 *   triple[3 h + k] = the index idx of :170 for draw k of iteration h (into the correspondences, not into pKF1's slots)
 *   n_its <= sind_sim3_iterations(n, ...): the caller may pass fewer
 * Outputs, per iteration h: count[h] = mnInliersi, inlier_bits[h * ceil(n / 64) + (i >> 6)] bit (i & 63) = mvbInliersi[i], s12[h] = ms12i, R12 = mR12i
 * (row-major), t12 = mt12i; mT12i is [s12 * R12 | t12] in FP32.  A degenerate sample (NaN hypothesis) has count 0, as every comparison in the reference fails.
 * ComputeSim3 runs on the host (csrc/host/sim3.cpp: FP64 libm calls, restated from OpenCV 4.2.0, parity unpinned), CheckInliers on the device in one launch
 * (csrc/match_sim3.hip).
 * Limits: n <= min(cap_last, cap_cur), n_its <= 300, B <= max_batch: beyond them SIND_E_CAPACITY.  A NULL array with a non-zero count, a triple index outside
 * [0, n) or a sigma2 that is negative or not finite -> SIND_E_ARG.  On an error nothing is launched and the outputs are untouched.  n_its = 0 and B = 0 are valid.
 *
 * sind_sim3_iterations = mRansacMaxIts after Sim3Solver::SetRansacParameters(probability, min_inliers, max_its) (:114-138; LoopClosing: 0.99, 20, 300) for n
 * correspondences; 0 if n < min_inliers, where iterate reports bNoMore at once (:146-150).  No handle, no device.
 */
typedef struct sind_sim3_item {
    const float* T1w; const float* T2w;                 /* poses of pKF1 / pKF2, 4x4 row-major, rows 0..2 read */
    int n; const float* x3Dw1; const float* x3Dw2;      /* the correspondences that survive :64-79, in i1 order: [n][3] each */
    const float* sigma2_1; const float* sigma2_2;       /* mvLevelSigma2[kp.octave] per correspondence */
    int n_its; const int* triple;                       /* [n_its][3] indices into 0..n-1 */
    int* count; uint64_t* inlier_bits;                  /* outputs (host): [n_its], [n_its][ceil(n / 64)] */
    float* s12; float* R12; float* t12;                 /* [n_its], [n_its][9], [n_its][3] */
} sind_sim3_item;
int sind_match_sim3_ransac(sind_match* m, const sind_sim3_item* items, int B, int fix_scale);
int sind_sim3_iterations(int n, double probability, int min_inliers, int max_its);

/* sind_match_pnp_ransac.  Replaces, for B relocalisation candidates at once and for all of their RANSAC iterations, the arithmetic of
 *   double PnPsolver::compute_pose(double R[3][3], double t[3])           src/PnPsolver.cc:477-525 and everything it calls (:375-950): EPnP
 *   void PnPsolver::CheckInliers()                                        :308-339
 *   bool PnPsolver::Refine()                                              :260-305
 * (Tracking::Relocalization, src/Tracking.cc:1347-1540: the solver between sind_match_by_bow and sind_match_by_projection_kf).  In PnPsolver::iterate
 * (:165-258) the sample of an iteration depends only on the random stream and on N, so the caller draws every sample beforehand; this call evaluates all of
 * them ON THE DEVICE (csrc/match_pnp.hip; csrc/host/epnp.hpp is one source for host and device, FP64, restated from OpenCV 4.2.0, parity unpinned: see that
 * header), finds on the host which Refine problems the reference would solve, and evaluates those as well.  iterate's bookkeeping is a replay over `count`
 * and `refine` (INTEGRATION.md gives it in C++, sindslam_amd/pnp.py in Python).  Runs on the sind_match handle.
 * Calibration: fu fv uc vc are the handle's fx fy cx cy, read as the FP64 of the FP32 the handle holds (PnPsolver: `fu = F.fx`, a double member from a float).
 * The constructor (:67-110) stays with the caller, flattened: per correspondence, i.e. per keypoint i with pMP && !pMP->isBad(), in ascending i (the caller
 * keeps mvKeyPointIndices):  p2d = F.mvKeysUn[i].pt, sigma2 = F.mvLevelSigma2[kp.octave] (finite, >= 0), x3Dw = pMP->GetWorldPos().
 *   th2, min_inliers: mvMaxError[i] = sigma2[i] * th2 (a float product) and mRansacMinInliers AFTER SetRansacParameters (sind_pnp_ransac_params); min_inliers >= 1
 *   samples[4 h + k] = the index idx of :195 for draw k of iteration h (into the correspondences); the four of an iteration are distinct
 *   best_count, best_bits = mnBestInliers and mvbBestInliers the solver holds from earlier calls (0 and NULL: none); best_bits has best_count bits set
 * Outputs, per iteration h: count[h] = mnInliersi, inlier_bits[h * ceil(n / 64) + (i >> 6)] bit (i & 63) = mvbInliersi[i], R (row-major) = mRi, t = mti,
 * refine[h] = the row of the refine outputs that holds what Refine() computes in iteration h, -1 if count[h] < min_inliers (no Refine).
 * Per refine r < *n_refines (at most n_its + 1 rows): refine_hyp[r] = the iteration whose inlier set it refines, -1 for best_bits; refine_count, refine_bits,
 * refine_R, refine_t = mnRefinedInliers, mvbRefinedInliers, mRi, mti after Refine()'s compute_pose and CheckInliers.  Refine() returns true iff
 * refine_count > min_inliers; mBestTcw / mRefinedTcw are R, t converted to FP32.  A NaN pose has count 0, as every comparison in the reference fails.
 * The refine problems are solved PNP_REFINE_SLOTS at a time; more of them means further rounds inside the call, not an error.
 * Limits: n <= min(cap_last, cap_cur), n_its <= 300, B <= max_batch: beyond them SIND_E_CAPACITY.  A NULL array with a non-zero count, a sample index outside
 * [0, n), a repeated index inside a sample, a sigma2 that is negative or not finite, min_inliers < 1, or a best_count that is not the number of bits set in
 * best_bits -> SIND_E_ARG.  On an error nothing is launched and the outputs are untouched.  n_its = 0 and B = 0 are valid: a call in which no item has an iteration writes nothing;
 * in a call in which some item has, an item with n_its = 0 gets *n_refines = 0 (if n_refines is not NULL) and nothing else.
 *
 * sind_pnp_ransac_params = mRansacMinInliers and mRansacMaxIts after PnPsolver::SetRansacParameters(probability, min_inliers, max_its, min_set, epsilon, th2)
 * (:121-157; the header's defaults 0.99, 8, 300, 4, 0.4, 5.991; Relocalization: 0.99, 10, 300, 4, 0.5, 5.991) for n > 0 correspondences.  No handle, no device.
 */
typedef struct sind_pnp_item {
    int n; const float* x3Dw; const float* p2d; const float* sigma2;   /* the correspondences: [n][3], [n][2], [n] */
    float th2; int min_inliers;
    int n_its; const int* samples;                      /* [n_its][4] indices into 0..n-1 */
    int best_count; const uint64_t* best_bits;          /* [ceil(n / 64)] or NULL */
    int* count; uint64_t* inlier_bits;                  /* outputs (host): [n_its], [n_its][ceil(n / 64)] */
    double* R; double* t; int* refine;                  /* [n_its][9], [n_its][3], [n_its] */
    int* n_refines; int* refine_hyp; int* refine_count; /* [1], [n_its + 1], [n_its + 1] */
    uint64_t* refine_bits; double* refine_R; double* refine_t;   /* [n_its + 1][ceil(n / 64)], [n_its + 1][9], [n_its + 1][3] */
} sind_pnp_item;
int sind_match_pnp_ransac(sind_match* m, const sind_pnp_item* items, int B);
void sind_pnp_ransac_params(int n, double probability, int min_inliers, int max_its, int min_set, float epsilon, int* min_inliers_out, int* max_its_out);

/* sind_match_pose_optimize.  Replaces, for B frames (or relocalisation candidates) at once, the whole of
 *   int Optimizer::PoseOptimization(Frame *pFrame)                        src/Optimizer.cc:239-451
 * (Tracking::TrackReferenceKeyFrame, TrackWithMotionModel, TrackLocalMap: src/Tracking.cc:812, 935, 977; Relocalization: :1477, 1493, 1508): the g2o graph of one
 * VertexSE3Expmap and N EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose with Huber kernels, OptimizationAlgorithmLevenberg over LinearSolverDense, the
 * four rounds of ten iterations from the input pose and the outlier classification between them, ONE launch for all items (csrc/match_pose.hip, one workgroup
 * per item; csrc/host/pose_opt.hpp is one FP64 source for host and device).  H, b and the robust chi2 are g2o's sums: every entry added in ascending edge order.
 * Calibration: fx fy cx cy bf are the handle's, read as the FP64 of the FP32 it holds (`e->fx = pFrame->fx`).  Runs on the sind_match handle.
 * What stays with the caller is the flattening (:280-360): per keypoint i with pFrame->mvpMapPoints[i] != NULL, in ascending i (PoseOptimization does not test
 * isBad; the caller keeps the index list and scatters `outlier` back into mvbOutlier):  x3Dw = pMP->GetWorldPos(), obs_xy = mvKeysUn[i].pt, u_right = mvuRight[i]
 * (< 0: the monocular edge), inv_sigma2 = mvInvLevelSigma2[kpUn.octave] (finite, >= 0); Tcw = pFrame->mTcw (finite).  And pFrame->SetPose(Tcw_out) afterwards.
 * Outputs: Tcw_out = the matrix SetPose gets; outlier[i] = mvbOutlier of the correspondence; *n_good = nInitialCorrespondences - nBad.  n < 3: *n_good = 0,
 * *n_rounds = 0 and NOTHING else is written (the reference returns before SetPose).  n < 10: one round only (:440).  The round arrays may be NULL; rounds that
 * did not run keep zeros: round_iters = optimize()'s return, round_nbad = nBad after the round, round_pose = [R row-major | t] of the vertex, round_chi2 =
 * activeRobustChi2 after the round's last accepted step, round_lambda = _currentLambda at its end.
 * Unpinned: parity with a real g2o / Eigen build (Eigen's evaluation order in the small products, its LDLT, the reference's -march=native contraction, and sin / cos /
 * pow, which pose_opt.hpp defines instead of calling a maths library); see the head of that file, also for the two places where the reference reads state it never set.
 * Limits: n <= min(cap_last, cap_cur), B <= max_batch: beyond them SIND_E_CAPACITY.  A NULL array with n > 0 (Tcw, Tcw_out, n_good, n_rounds always), an inv_sigma2 that
 * is negative or not finite, a pose that is not finite -> SIND_E_ARG.  On an error nothing is launched and the outputs are untouched.  B = 0 and n = 0 are valid.
 */
typedef struct sind_poseopt_item {
    int n; const float* x3Dw; const float* obs_xy; const float* u_right; const float* inv_sigma2;  /* [n][3], [n][2], [n] (< 0: monocular edge), [n] */
    const float* Tcw;                                   /* [16] row-major: pFrame->mTcw on entry */
    float* Tcw_out; uint8_t* outlier; int* n_good;      /* [16] = the pose SetPose gets; [n] = mvbOutlier; nInitialCorrespondences - nBad */
    int* n_rounds; int* round_iters; int* round_nbad;   /* [1]; [4] optimize()'s return per round; [4] */
    double* round_pose; double* round_chi2; double* round_lambda;  /* [4][12] R row-major | t after the round; [4] activeRobustChi2 after its last accepted step; [4] _currentLambda at its end */
} sind_poseopt_item;
int sind_match_pose_optimize(sind_match* m, const sind_poseopt_item* items, int B);

/* sind_match_sim3_optimize.  Replaces, for B loop candidates at once, the whole of
 *   int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)
 * (src/Optimizer.cc:1046-1241; LoopClosing::ComputeSim3, src/LoopClosing.cc:300): the g2o graph of one VertexSim3Expmap and, per correspondence, two fixed points and
 * the edges EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ with Huber kernels (delta = the float sqrt(th2)), their NUMERIC Jacobians (the reference has no analytic
 * ones: central differences with 1e-9), OptimizationAlgorithmLevenberg over LinearSolverDense, optimize(5), the bad pairs removed, optimize(5 or 10) from where the
 * first stage stopped, the final classification.  ONE launch for all items (csrc/match_sim3opt.hip, one workgroup per item; csrc/host/sim3_opt.hpp is one FP64
 * source for host and device).  H, b and the robust chi2 are g2o's sums: every entry added in edge order (e12 of pair 0, e21 of pair 0, e12 of pair 1, ...).
 * What stays with the caller is the flattening (:1099-1178): per index i with vpMatches1[i] != NULL, pKF1's map point i and the match both non-NULL and not bad and
 * the match seen in pKF2 (i2 >= 0), in ascending i: x3Dc1 = R1w * P3D1w + t1w and x3Dc2 = R2w * P3D2w + t2w in FP32 (as for sind_match_sim3_ransac), obs1_xy =
 * pKF1->mvKeysUn[i].pt, obs2_xy = pKF2->mvKeysUn[i2].pt, inv_sigma2_1 / _2 = mvInvLevelSigma2[octave] of the two (finite, >= 0), K1 / K2 = fx fy cx cy of the two key
 * frames, s12 R12 t12 = what g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) gets (finite).  The caller keeps the index list and nulls
 * vpMatches1[idx] where removed is 1.
 * Outputs: q_out (x y z w, NOT normalised: g2o::Sim3 never normalises), t_out, s_out = g2oS12 afterwards in FP64, equal to the input (Quaterniond(R12), t12, s12) when 0
 * is returned early; removed[i] = 1 where either classification nulled the match; *n_inliers = the return value.  n = 0: the empty graph, 0 returned, nothing else
 * happens.  1 <= n and fewer than 10 pairs left after the first stage: the first stage has run and removed is set, 0 returned, the Sim3 stays the input.
 * The diagnostics may be NULL: n_bad = nBad of the first stage, n_stages = stages run (0, 1, 2), stage_iters = optimize()'s return, stage_chi2 = activeRobustChi2 after
 * the stage's last accepted step, stage_lambda = _currentLambda at its end; a stage that did not run keeps zeros.
 * fix_scale: VertexSim3Expmap::_fix_scale (mbFixScale: true for stereo / RGB-D).  th2: 10 in LoopClosing.
 * Unpinned: parity with a real g2o / Eigen build (Eigen's evaluation order in Sim3's exponential and the small products, its LDLT, -march=native contraction, and
 * sin / cos / exp, which pose_opt.hpp and sim3_opt.hpp define instead of calling a maths library); see the head of sim3_opt.hpp.
 * Limits: n <= min(cap_last, cap_cur), B <= max_batch: beyond them SIND_E_CAPACITY.  A NULL array (with n = 0 the per-pair arrays may be NULL), an inv_sigma2 that is
 * negative or not finite, an input Sim3, intrinsic or th2 that is not finite -> SIND_E_ARG.  On an error nothing is launched and the outputs are untouched.  B = 0 is valid.
 */
typedef struct sind_sim3opt_item {
    int n; float s12;                                    /* pairs; the input scale */
    const float* x3Dc1; const float* x3Dc2;              /* [n][3] the points in their own cameras */
    const float* obs1_xy; const float* obs2_xy;          /* [n][2] */
    const float* inv_sigma2_1; const float* inv_sigma2_2;/* [n] */
    const float* K1; const float* K2;                    /* [4] fx fy cx cy */
    const float* R12; const float* t12;                  /* [9] row-major, [3] */
    double* q_out; double* t_out; double* s_out;         /* [4] x y z w, [3], [1] */
    uint8_t* removed; int* n_inliers;                    /* [n]; [1] */
    int* n_bad; int* n_stages; int* stage_iters;         /* [1]; [1]; [2] */
    double* stage_chi2; double* stage_lambda;            /* [2]; [2] */
} sind_sim3opt_item;
int sind_match_sim3_optimize(sind_match* m, const sind_sim3opt_item* items, int B, float th2, int fix_scale);

/* sind_match_local_ba.  Replaces, for B local windows at once, the whole of
 *   void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool* pbStopFlag, Map* pMap)
 * from the optimizer's set-up on (src/Optimizer.cc:506-743; LocalMapping::Run, src/LocalMapping.cc:100): the g2o graph of the local key frames (free, the one with
 * mnId 0 fixed), the fixed cameras and the local map points (marginalised), one EdgeSE3ProjectXYZ or EdgeStereoSE3ProjectXYZ with a Huber kernel per observation,
 * BlockSolver_6_3's Schur complement under OptimizationAlgorithmLevenberg, optimize(5), the outliers moved to level 1 and the kernels removed, optimize(10), the final
 * classification.  ONE launch for all items (csrc/match_localba.hip, one workgroup per item; csrc/host/local_ba.hpp over csrc/host/ba_schur.hpp is one FP64 source for host and device and states
 * the order of every sum).  Calibration is the handle's fx fy cx cy bf, as for sind_match_pose_optimize.
 * What stays with the caller: the graph collection (:455-504: lLocalKeyFrames, lLocalMapPoints, lFixedCameras; sindslam_amd/optimizer.py mirrors it), and after the
 * call, under the map mutex, EraseMapPointMatch and EraseObservation for every erased observation (:748-757), SetPose (:762-768), SetWorldPos and
 * UpdateNormalAndDepth (:771-777; sind_match_update_points below does the latter for all points in one call).
 * Inputs: kf_kind 0 = a local key frame, 1 = a local key frame that is fixed (mnId == 0), 2 = a fixed camera; Tcw = GetPose(); the points in lLocalMapPoints order
 * with x3Dw = GetWorldPos(); the observations of point j are obs_start[j] .. obs_start[j + 1] - 1 in the order the edges are added (key frames that are bad left out):
 * obs_kf the index of the key frame in 0 .. n_kf - 1, obs_xy = mvKeysUn[slot].pt, u_right = mvuRight[slot] (< 0: the monocular edge), inv_sigma2 =
 * mvInvLevelSigma2[octave].  In the reference the order of a point's observations is that of a std::map keyed by pointers, which no caller can reproduce; the
 * Python mirror uses ascending mnId.  do_more = 0 is bDoMore = false (the stop flag seen after the first optimize): no level changes and no second stage.
 * Outputs: Tcw_out = toCvMat(estimate) for kinds 0 and 1 (a round trip through the quaternion, for the fixed one too), the input for kind 2; x3Dw_out = the float of
 * the estimate; erase[k] = 1 where observation k is in vToErase.  The diagnostics may be NULL: n_stages = the optimize calls that had something to optimise (0..2),
 * stage_iters = their return values, n_level1 = the edges at level 1 after the first classification, stage_chi2 = activeRobustChi2 after the stage's last accepted
 * step, stage_lambda = _currentLambda at its end; a stage that did not run keeps zeros.
 * Valid: B = 0; n_obs = 0 (initializeOptimization refuses an empty graph and nothing is optimised: the outputs are the conversions alone).
 * Unpinned: parity with a real g2o / Eigen build, above all the reduced system (a dense LDL^T in natural order here, SimplicialLDLT under AMD ordering there); see the
 * head of ba_schur.hpp.  Not offered: a stop flag that flips in the middle of an optimize.
 * Limits: 256 key frames of kind 0, 4096 key frames, 65536 points, 2^20 observations, 2^24 entries of the co-observation lists (sum over the points of k (k + 1) / 2,
 * k = its observations in key frames of kind 0), B <= max_batch: beyond them SIND_E_CAPACITY.  The workspace lives on the handle, grows between calls to the largest
 * call seen and is freed with the handle.
 * SIND_E_ARG: a NULL array with a non-zero count, ids that repeat, a kind outside 0..2, an obs_kf out of range, the same key frame twice in one point's observations, an
 * obs_start that does not start at 0 or decreases, an inv_sigma2 that is negative or not finite, a pose or point that is not finite, no key frame of kind 0.  On an
 * error nothing is launched and the outputs are untouched.
 */
typedef struct sind_localba_item {
    int n_kf; const int64_t* kf_id; const uint8_t* kf_kind;   /* [n_kf]; 0 local, 1 local and fixed (mnId == 0), 2 fixed camera */
    const float* Tcw;                                         /* [n_kf][16] GetPose() */
    int n_mp; const int64_t* mp_id; const float* x3Dw;        /* [n_mp], [n_mp][3]; in lLocalMapPoints order */
    const int* obs_start;                                     /* [n_mp + 1]: the observations of point j, in the order the edges are added */
    const int* obs_kf;                                        /* [n_obs] index into 0..n_kf-1 */
    const float* obs_xy; const float* u_right; const float* inv_sigma2;   /* [n_obs][2], [n_obs] (< 0: mono), [n_obs] */
    int do_more;
    float* Tcw_out; float* x3Dw_out; uint8_t* erase;          /* [n_kf][16] (kind 2 rows: the input), [n_mp][3], [n_obs] = vToErase */
    int* n_stages; int* stage_iters; int* n_level1;           /* diagnostics, may be NULL: [1], [2], [1] */
    double* stage_chi2; double* stage_lambda;                 /* [2], [2] */
} sind_localba_item;
int sind_match_local_ba(sind_match* m, const sind_localba_item* items, int B);
int sindh_local_ba(const sind_localba_item* items, int B, const float* K5);   /* host twin (libsind_host.so too): K5 = fx fy cx cy bf */

/* sind_match_essential_graph.  Replaces, for B pose graphs at once, the whole of
 *   void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose &NonCorrectedSim3, const KeyFrameAndPose &CorrectedSim3,
 *                                          const map<KeyFrame *, set<KeyFrame *> > &LoopConnections, const bool &bFixScale)
 * from the optimizer's set-up on (src/Optimizer.cc:787-1043; LoopClosing::CorrectLoop, src/LoopClosing.cc:567): one VertexSim3Expmap per key frame (pLoopKF fixed), one
 * EdgeSim3 with the identity as information per edge, OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16), optimize(20), the recovery of every key frame's
 * SE3 pose (:999-1009) and the correction of every map point through its reference key frame (:1020-1040).  TWO launches on one stream with one host wait
 * (csrc/match_essgraph.hip: k_ess_graph, one workgroup per item, then k_ess_points over the points of all items; csrc/host/essential_graph.hpp is one FP64 source for
 * host and device and states the order of every sum).
 * What stays with the caller: which edges exist (:853-983: the minFeat = 100 weights and the (cur, loop) exception, sInsertedEdges, parent, hasChild, sLoopEdges and
 * the mnId comparisons; sindslam_amd/optimizer.py mirrors the collection) and, under the map mutex, SetPose, SetWorldPos and UpdateNormalAndDepth with the outputs
 * (sind_match_update_points below does the latter for all points in one call).
 * Inputs: the key frames in ascending mnId (kf_id), Tcw = GetPose(); has_corrected / corrected = the CorrectedSim3 entry of the key frame (qx qy qz qw tx ty tz s),
 * has_noncorrected / noncorrected = its NonCorrectedSim3 entry; fixed_kf = the index of pLoopKF.  vScw[i] is the corrected entry if present, else Sim3(Rcw, tcw, 1.0).
 * The edges in the order the reference adds them: edge_i is vertex 0 and edge_j vertex 1; edge_kind 0 = a LoopConnections edge, its measurement Sjw * Swi from vScw of
 * both ends (:857-872); edge_kind 1 = a spanning-tree, loop or covisibility edge, both ends from the non-corrected Sim3 where one exists, else vScw (:889-979).  Several
 * edges may join the same two key frames (LoopConnections holds both directions): their blocks add in edge order.  The map points that are not bad: x3Dw =
 * GetWorldPos(), mp_ref = the index of the key frame of nIDr (mnCorrectedReference if mnCorrectedByKF == pCurKF->mnId, else the reference key frame).
 * Outputs: Siw_out = the vertex estimates after optimize(20) (the input estimate of the fixed vertex and of a vertex without edges); Tiw_out =
 * toCvSE3(q.toRotationMatrix(), t * (1. / s)); x3Dw_out = the float of Siw_out[ref].inverse().map(vScw[ref].map(P)).  The diagnostics may be NULL: n_iters =
 * optimize's return (-1 where nothing was optimised), chi2 = activeChi2 after the last accepted step, lambda = _currentLambda at the end (-1 where nothing was
 * optimised), n_active = the vertices with a Hessian index, solver_fail = the factorisations that failed.
 * Valid: B = 0; n_edges = 0 (the empty graph: nothing is optimised, the outputs are the conversions alone); n_mp = 0; free vertices without edges.
 * Unpinned: parity with a real g2o / Eigen build: the linear system (a natural-order envelope LDL^T here, SimplicialLDLT under AMD ordering there), W.lu().solve(t) of
 * Sim3::log, std::log and acos (restated from fdlibm), the reference's iteration by pointer value; see the head of essential_graph.hpp.  Not offered: a stop flag.
 * Limits: 4096 key frames, 65536 edges, 2^20 points, 2^24 stored entries of the factor's envelope (sum over the free key frames with an edge, in ascending mnId with
 * rank I, of 49 (I - first(I) + 1), first(I) the smallest rank among I and its neighbours), B <= max_batch: beyond them SIND_E_CAPACITY.  The workspace lives on the
 * handle, grows between calls to the largest call seen and is freed with the handle.
 * SIND_E_ARG: a NULL array with a non-zero count, a negative count, kf_id not strictly ascending, fixed_kf or an edge end or an mp_ref out of range, edge_i == edge_j,
 * a kind outside 0..1, a pose, Sim3 or point that is not finite, a scale <= 0.  On an error nothing is launched and the outputs are untouched.
 */
typedef struct sind_essgraph_item {
    int n_kf; const int64_t* kf_id; const float* Tcw;                  /* [n_kf] strictly ascending; [n_kf][16] GetPose() */
    const uint8_t* has_corrected; const double* corrected;            /* [n_kf]; [n_kf][8] qx qy qz qw tx ty tz s (read where the flag is set) */
    const uint8_t* has_noncorrected; const double* noncorrected;      /* [n_kf]; [n_kf][8] */
    int fixed_kf;                                                      /* index of pLoopKF */
    int n_edges; const int* edge_i; const int* edge_j; const uint8_t* edge_kind;   /* [n_edges] vertex 0, vertex 1, 0 LoopConnections / 1 normal */
    int n_mp; const float* x3Dw; const int* mp_ref;                    /* [n_mp][3], [n_mp] index into 0..n_kf-1 */
    double* Siw_out; float* Tiw_out; float* x3Dw_out;                  /* [n_kf][8], [n_kf][16], [n_mp][3] */
    int* n_iters; double* chi2; double* lambda; int* n_active; int* solver_fail;   /* diagnostics, may be NULL: [1] each */
} sind_essgraph_item;
int sind_match_essential_graph(sind_match* m, const sind_essgraph_item* items, int B, int fix_scale);
int sindh_essential_graph(const sind_essgraph_item* items, int B, int fix_scale);   /* host twin (libsind_host.so too) */

/* sind_match_global_ba.  Replaces the whole of
 *   void Optimizer::BundleAdjustment(const vector<KeyFrame *> &vpKFs, const vector<MapPoint *> &vpMP, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF,
 *                                    const bool bRobust)
 * from the optimizer's set-up on (src/Optimizer.cc:49-191; GlobalBundleAdjustemnt forwards to it; LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:645): one
 * VertexSE3Expmap per key frame (fixed iff mnId == 0), one marginalised VertexSBAPointXYZ per point, one EdgeSE3ProjectXYZ or EdgeStereoSE3ProjectXYZ per observation,
 * Huber kernels only if robust (deltas the floats sqrt(5.99) and sqrt(7.815): the monocular one is not local BA's sqrt(5.991)), BlockSolver_6_3's Schur complement under
 * OptimizationAlgorithmLevenberg, initializeOptimization(), ONE optimize(iterations); no levels and no classification.  A global BA is one large item, so the phases
 * of the algorithm are KERNELS OVER THE WHOLE GRID, one element per lane, on the handle's stream (csrc/match_globalba.hip), stream order the only synchronisation, and
 * the Levenberg-Marquardt control flow runs on the host with one wait per linearisation and one per trial; no cooperative launch, no grid-wide flags, no atomics.
 * csrc/host/global_ba.hpp over csrc/host/ba_schur.hpp is one FP64 source for host and device; ba_schur.hpp states the order of every sum, once for both bundle adjustments, with the reduced camera system stored and
 * factored as a natural-order envelope in 6 x 6 block rows.  The B items of a call run one after the other.  Calibration is the handle's fx fy cx cy bf.
 * What stays with the caller: the collection of the graph (:68-184; sindslam_amd/optimizer.py mirrors it) and what follows the optimize (:193-235: SetPose / SetWorldPos
 * or mTcwGBA / mPosGBA, and UpdateNormalAndDepth, which sind_match_update_points below does for all points in one call), and the tail of RunGlobalBundleAdjustment
 * (sindslam_amd/optimizer.py: run_global_bundle_adjustment).
 * Inputs: the key frames that are not bad in ascending mnId (kf_id), Tcw = GetPose(); the points that are not bad, x3Dw = GetWorldPos(); the observations of point j are
 * obs_start[j] .. obs_start[j + 1] - 1 in the order the edges are added, those in bad key frames or in key frames the call does not hold left out (:109): obs_kf the
 * index of the key frame, obs_xy = mvKeysUn[slot].pt, u_right = mvuRight[slot] (< 0: the monocular edge), inv_sigma2 = mvInvLevelSigma2[octave].  iterations: the
 * reference passes 10 (loop closing) or 20 (the default); 0 is the stop flag already set at entry (no iteration; the outputs are the conversions alone).
 * Outputs: Tcw_out = toCvMat(estimate) of every key frame (a round trip through the quaternion, for the fixed one and for one without edges too); x3Dw_out = the float of
 * the estimate, the input for a point without observations (vbNotIncludedMP, :175-179); included[j] = 0 exactly for those points.  The diagnostics may be NULL: n_iters
 * = optimize's return (-1 where nothing was optimised), chi2 = activeRobustChi2 after the last accepted step, lambda = _currentLambda at the end (-1 before
 * computeLambdaInit), n_active_poses = the key frames with a Hessian index, solver_fail = the factorisations that failed, env_entries = the stored entries of the
 * factor's envelope, env_dense_entries = those of the dense lower triangle in 6 x 6 blocks, 36 n (n + 1) / 2.
 * Valid: B = 0; no key frame but mnId 0 (only the points move); no observations (nothing is optimised); n_mp = 0; no key frame with mnId 0 (nothing is fixed).
 * Unpinned: parity with a real g2o / Eigen build, above all the reduced system (a natural-order envelope LDL^T here, SimplicialLDLT under AMD ordering there) and the
 * order of a point's observations (a std::map keyed by pointers there); see the heads of ba_schur.hpp and global_ba.hpp.  Not offered: a stop flag that flips in the
 * middle of the optimize.
 * Limits: 4096 key frames, 2^20 points, 2^22 observations, 2^26 entries of the co-observation lists (sum over the points of k (k + 1) / 2, k = its observations in key
 * frames with mnId != 0), 2^25 stored entries of the envelope (sum over the key frames with a Hessian index I of 36 (I - first(I) + 1), first(I) the smallest index among
 * I and the key frames that share a point with it), B <= max_batch: beyond them SIND_E_CAPACITY, decided before anything is allocated or launched.  The workspace lives
 * on the handle, grows between calls to the largest call seen and is freed with the handle.
 * SIND_E_ARG: a NULL array with a non-zero count, a negative count or iteration count, kf_id not strictly ascending, point ids that repeat, an obs_kf out of range, the
 * same key frame twice in one point's observations, an obs_start that does not start at 0 or decreases, an inv_sigma2 that is negative or not finite, a pose or point
 * that is not finite.  On an error nothing is launched and the outputs are untouched.
 */
typedef struct sind_globalba_item {
    int n_kf; const int64_t* kf_id; const float* Tcw;         /* [n_kf] strictly ascending; [n_kf][16] GetPose() */
    int n_mp; const int64_t* mp_id; const float* x3Dw;        /* [n_mp], [n_mp][3] */
    const int* obs_start;                                     /* [n_mp + 1]: the observations of point j, in the order the edges are added */
    const int* obs_kf;                                        /* [n_obs] index into 0..n_kf-1 */
    const float* obs_xy; const float* u_right; const float* inv_sigma2;   /* [n_obs][2], [n_obs] (< 0: mono), [n_obs] */
    float* Tcw_out; float* x3Dw_out; uint8_t* included;       /* [n_kf][16], [n_mp][3], [n_mp] */
    int* n_iters; double* chi2; double* lambda; int* n_active_poses; int* solver_fail;   /* diagnostics, may be NULL: [1] each */
    long long* env_entries; long long* env_dense_entries;     /* [1] each */
} sind_globalba_item;
int sind_match_global_ba(sind_match* m, const sind_globalba_item* items, int B, int iterations, int robust);
int sind_match_global_ba_counts(sind_match* m, long long* launches, long long* waits);   /* of the last sind_match_global_ba on the handle: kernel launches, host waits */
int sindh_global_ba(const sind_globalba_item* items, int B, int iterations, int robust, const float* K5);   /* host twin (libsind_host.so too): K5 = fx fy cx cy bf */

/* Map-point upkeep on the matcher handle (csrc/capi_match_map.cpp, csrc/match_mappoints.hip; csrc/host/map_points.hpp is one source for host and device and states
 * the type of every step).
 *
 * sind_match_triangulate.  Replaces, for B (current key frame, neighbour) pairs at once, the per-match loop of
 *   void LocalMapping::CreateNewMapPoints()                                                             src/LocalMapping.cc:284-431
 *   cv::Mat KeyFrame::UnprojectStereo(int i)                                                            src/KeyFrame.cc:615-631
 * from the ray parallax to the scale-consistency test: ONE launch, one lane per match over the matches of all pairs (k_tri_points), everything of a match in registers.
 * fx fy cx cy bf, scale_factors and nlevels are the handle's: invfx = 1.0f / fx, mb = bf / fx, mvLevelSigma2[l] = scale[l] * scale[l], ratioFactor = 1.5f * scale[1],
 * all in FP32.  Capacities: kf1.n <= cap_last, kf2.n <= cap_cur, B <= max_batch.
 * What stays with the caller: the neighbours and the baseline test (:213-261), ComputeF12 and sind_match_for_triangulation before the call; after it, for every
 * status 0 in (pair, idx1) order, new MapPoint, both AddObservation, both AddMapPoint and the list (:434-449), then sind_match_update_points over the new points
 * (sindslam_amd/mapping.py: create_new_map_points does all of it on plain dicts).
 * Inputs: Tcw1 / Twc1 = GetPose() / GetPoseInverse() of the current key frame, Tcw2 / Twc2 of the neighbour, 4x4 row-major, rows 0..2 are read (Ow = column 3 of Twc;
 * Rwc of the rays = the transpose of Tcw's rotation, the rotation of UnprojectStereo = Twc's, as there); per key frame and keypoint xy = mvKeys[i].pt (the distorted
 * key, read by UnprojectStereo), un_xy = mvKeysUn[i].pt, octave = mvKeysUn[i].octave, u_right = mvuRight, depth = mvDepth; match12 [kf1.n] exactly as
 * sind_match_for_triangulation writes it.  The matches are walked in ascending idx1, the order of vMatchedIndices.
 * Outputs, [kf1.n] like match12: x3D (the point where one was formed, else zeros), how (0 triangulated by the 4x4 SVD, 1 UnprojectStereo of key frame 1, 2 of key
 * frame 2, -1 none), status: 0 a new point; 1 no stereo and low parallax (:349); 2 w == 0 (:333); 3 z1 <= 0; 4 z2 <= 0; 5 reprojection in key frame 1; 6 in key frame 2;
 * 7 a zero distance; 8 scale inconsistency; -1 where match12 < 0 (x3D zeros, how -1).  *nnew = the entries with status 0.
 * cos(2 * atan2(mb / 2, depth)) is evaluated with the float overloads of the C library ON THE HOST inside the call, once per match with a stereo side, and never on the
 * device; the kernel receives the cosine.
 * Valid: B = 0; pairs without matches; kf1.n = 0.
 * Unpinned: parity with a real OpenCV build (the 4x4 SVD is OpenCV 4.2's JacobiSVDImpl_<float> restated; the small-matrix conventions of csrc/match_local.hip).
 * SIND_E_CAPACITY beyond the capacities.  SIND_E_ARG: a NULL array with a non-zero count, a match12 entry outside [-1, kf2.n), an octave outside [0, nlevels), a pose
 * that is not finite, a matched keypoint with u_right >= 0 and depth <= 0 (the reference's UnprojectStereo returns an empty matrix there and the loop goes on to read
 * it).  On an error nothing is launched and the outputs are untouched.
 */
typedef struct sind_tri_side { int n; const float* xy; const float* un_xy; const int* octave; const float* u_right; const float* depth; } sind_tri_side;   /* [n][2] x2, [n] x3 */
typedef struct sind_tri_pair {
    const float* Tcw1; const float* Twc1; const float* Tcw2; const float* Twc2;      /* [16] each */
    sind_tri_side kf1, kf2;
    const int* match12;                                                               /* [kf1.n]: idx2 or -1 */
    float* x3D; int* how; int* status; int* nnew;                                     /* outputs (host): [kf1.n][3], [kf1.n], [kf1.n], [1] */
} sind_tri_pair;
int sind_match_triangulate(sind_match* m, const sind_tri_pair* pairs, int B);
/* host twin (libsind_host.so too): K5 = fx fy cx cy bf; no capacities */
int sindh_triangulate(const sind_tri_pair* pairs, int B, const float* K5, const float* scale_factors, int nlevels);

/* sind_match_update_points.  Replaces, for every point of B lists at once,
 *   void MapPoint::ComputeDistinctiveDescriptors()                                                      src/MapPoint.cc:242-307
 *   void MapPoint::UpdateNormalAndDepth()                                                               src/MapPoint.cc:330-371
 * the pair the reference calls for every point of a new key frame (LocalMapping.cc:152-153), for every new point (:442-444), after Fuse (:526-527), after local BA
 * (Optimizer.cc:776), after the essential graph (:1042) and a global BA (:227) and in LoopClosing.cc:500, :532.  Its outputs are what sind_match_local_map, sind_match_fuse,
 * sind_match_by_projection_sim3 and sind_match_by_sim3 take per map point: desc, normal, max_dist, min_dist.  TWO launches on the handle's stream with one host wait:
 * k_mp_descriptor, one wave per point (all-pairs Hamming distances row by row, the row's median by bisection with wave ballots, nothing stored or sorted), and
 * k_mp_normal, one lane per point, which walks its list in order.  scale_factors and nlevels are the handle's.
 * What stays with the caller: isBad() of the point (a bad point is not passed), the locks, and writing the outputs to the map.
 * Inputs: Ow [n_kf][3] = GetCameraCenter() of the key frames the item's observations name; x3Dw [n_mp][3] = GetWorldPos(); the observations of point j are obs_start[j]
 * .. obs_start[j + 1] - 1 (the layout of sind_localba_item) in the order the caller's map iterates (the reference: a std::map keyed by pointers; the Python mirror:
 * ascending mnId): obs_kf the index into Ow, obs_bad = pKF->isBad(), obs_octave = mvKeysUn[slot].octave, obs_desc = the 32 bytes of mDescriptors.row(slot); ref_obs[j] =
 * the position of mpRefKF within point j's own list (0 .. count - 1; -1: not in it).  do_descriptor, do_normal: which of the two functions run.
 * Outputs.  Descriptor: only observations in key frames that are not bad enter, N their number; the median of a row is entry (int)(0.5 * (N - 1)) of its N sorted distances
 * (the zero to itself included); the FIRST row with the strictly smallest median wins.  best_obs[j] = its position in the point's list, desc_out[j] = its 32 bytes; where
 * the reference returns early (no observations, or every observer bad) best_obs[j] = -1 and desc_out[j] is untouched.  Normal: ALL observations enter the sum, those in bad
 * key frames too, as there; sequential FP32 in list order.  normal_out = mNormalVector, max_dist = mfMaxDistance, min_dist = mfMinDistance: the members, before the
 * 1.2f / 0.8f of GetMaxDistanceInvariance / GetMinDistanceInvariance, as the searches take them; updated[j] = 1, or 0 where the reference returns on empty observations
 * and the three are untouched.  With do_descriptor = 0 desc_out and best_obs are untouched (and may be NULL), with do_normal = 0 the other four.
 * Valid: B = 0; n_mp = 0; points without observations.
 * Unpinned: cv::norm and the MatExpr scalings (the conventions of csrc/match_local.hip).
 * Limits: 4096 key frames, 65536 points, 2^20 observations per item, B <= max_batch: beyond them SIND_E_CAPACITY.  No limit on the observations of one point below
 * these.  The workspace lives on the handle, grows between calls to the largest call seen and is freed with the handle.
 * SIND_E_ARG: a NULL array with a non-zero count, a negative count, an obs_start that does not start at 0 or decreases, an obs_kf, an obs_octave or a ref_obs out of
 * range, ref_obs = -1 on a point that has observations while do_normal is set (the reference would index a map entry that does not exist), a position or camera centre
 * that is not finite.  On an error nothing is launched and the outputs are untouched.
 */
typedef struct sind_mappoints_item {
    int n_kf; const float* Ow;                                                        /* [n_kf][3] */
    int n_mp; const float* x3Dw;                                                      /* [n_mp][3] */
    const int* obs_start;                                                             /* [n_mp + 1] */
    const int* obs_kf; const uint8_t* obs_bad; const int* obs_octave; const uint8_t* obs_desc;   /* [n_obs], [n_obs], [n_obs], [n_obs][32] */
    const int* ref_obs;                                                               /* [n_mp] */
    int do_descriptor, do_normal;
    uint8_t* desc_out; int* best_obs;                                                 /* outputs (host): [n_mp][32], [n_mp] */
    float* normal_out; float* max_dist; float* min_dist; uint8_t* updated;            /* [n_mp][3], [n_mp] x3 */
} sind_mappoints_item;
int sind_match_update_points(sind_match* m, const sind_mappoints_item* items, int B);
int sindh_update_points(const sind_mappoints_item* items, int B, const float* scale_factors, int nlevels);   /* host twin (libsind_host.so too); no limits */

/* ------------------------------------------------------------------------------------------------------------
 * Covisibility: the observations of the map on the device and the three walks over them.  Replaces the counting in
 *   void KeyFrame::UpdateConnections()                                                                  src/KeyFrame.cc:289-320
 *   void Tracking::UpdateLocalKeyFrames()                                                               src/Tracking.cc:1268-1288
 *   void LocalMapping::KeyFrameCulling()                                                                src/LocalMapping.cc:645-691
 * each of which copies every point's std::map<KeyFrame*, size_t> and counts per key frame.  A handle of its own (its own stream, fixed capacity from create), as
 * sind_bowdb: the state lives on the device and a query uploads point ids alone.  All arithmetic is integer: the results are the literal loops' in any order of
 * evaluation, and nothing here is unpinned but the order in which the CALLER walks pointer-keyed containers (the Python layer: ascending id).
 * State.  The point side of the map (MapPoint::mObservations) stored key-frame-major: cell (kf, idx), kf in [0, cap_kf), idx in [0, cap_feat), holds `point`
 * (-1: empty), `octave` = mvKeysUn[idx].octave and `stereo` = (mvuRight[idx] >= 0).  A point has at most one cell per key frame (AddObservation ignores a second
 * one): that is the caller's contract and is not checked.  Per point the handle keeps n_obs (the reference's nObs: a stereo cell counts 2) and a histogram of its
 * cells by octave, [nlevels].
 *   apply   n ops {kf, idx, point, octave, stereo} in ONE launch (k_covis_apply, one lane per op): the lane exchanges the cell and moves the two aggregates of the
 *           old and the new point with integer atomics.  point = -1 clears the cell (octave and stereo are not read); setting an occupied cell replaces its
 *           content; clearing an empty cell does nothing; n = 0 is valid.  A call may hold at most ONE op per cell (checked on the host), which keeps the
 *           exchange free of races.  The caller's array is free again on return.
 *   count   Q queries {self_kf, n, points, count} at once: count[k], k in [0, cap_kf), = the number of list entries whose point has a cell in key frame k.  An entry
 *           -1 is skipped (NULL, or a point the caller found isBad(): that filter is the caller's, as for sind_match_update_points).  count[self_kf] = 0 is the
 *           mnId == mnId skip of UpdateConnections; self_kf = -1 (the tracker's vote) skips nothing.  The list is a MULTISET: a point listed twice counts twice, as
 *           the loop over mvpMapPoints does.  THREE launches and one host wait for any Q: k_covis_tag (one lane per entry; every query owns as many consecutive bits
 *           of a per-point tag as its list names one point most often, bit t tagging the points named more than t times), k_covis_count (one wave per key-frame row
 *           and 64 bits: the row read coalesced, the tags gathered, one ballot and popcount per bit; no atomics), k_covis_untag (clears exactly the bits that were set;
 *           the tags are never cleared wholesale).  The bits of a query are added on the host.  The cost is one pass over rows * cap_feat cells per 64 bits, rows =
 *           the highest key frame ever set + 1, whatever the observation counts.
 *   cull    B items {kf, n, points, octave, close, n_mps, n_redundant, redundant} at once, each the body of the loop over one key frame's points in KeyFrameCulling,
 *           entry i = feature i of key frame kf.  An entry is skipped if its point is -1 or close[i] is 0 (close carries the mvDepth test of :660, which the caller
 *           evaluates; all 1 for monocular).  Otherwise *n_mps is incremented, and the entry is redundant if n_obs(point) > th_obs and the point has at least th_obs
 *           cells in OTHER key frames with octave <= octave[i] + 1: the histogram's prefix up to min(octave[i] + 1, nlevels - 1), minus the point's own cell in kf
 *           if it has one there that qualifies.  The own cell is (kf, i) where that holds the point; otherwise the row is searched (an inconsistent map may hold
 *           the point at another index, or at none).  The reference's early break makes its verdict depend on that count alone.  redundant[i] = 0 / 1 per
 *           entry (skipped: 0; may be NULL), *n_redundant their sum.  ONE launch (k_covis_cull, one lane per entry, the counts reduced per item) and one wait.
 *           What stays with the caller: nRedundantObservations > 0.9 * nMPs (:693, FP64) and SetBadFlag.
 *   read_row, read_points   the state back, for tests and tools: a row's cells (octave and stereo 0 where empty), and n_obs and the histogram of n points.
 * Limits, decided in create: cap_kf * cap_feat <= 2^28, cap_points <= 2^24, nlevels <= 16, max_queries <= 4096: beyond them SIND_E_CAPACITY.  Per call: a list or an
 * item of more than cap_feat entries, Q or B > max_queries, or more tag bits in one count than 64 * ceil(max_queries / 64): SIND_E_CAPACITY.
 * SIND_E_ARG: a NULL handle, a NULL array with a non-zero count, a NULL output, a negative count, a key frame, index, point or octave out of range (a point: [-1,
 * cap_points); self_kf: [-1, cap_kf); the octave of a skipped cull entry is not read), two ops on one cell.  On any error nothing is launched, the state and the outputs
 * are untouched.
 * sindh_covis_* are the host twins (libsind_host.so too): the same per-element source (csrc/host/covis.hpp), the state in host memory, none of the per-call limits.
 */
typedef struct sind_covis sind_covis;
typedef struct sind_covis_op { int kf, idx, point, octave, stereo; } sind_covis_op;
typedef struct sind_covis_query {
    int self_kf, n; const int* points;                                                /* [n] */
    int* count;                                                                       /* output (host), [cap_kf] */
} sind_covis_query;
typedef struct sind_covis_cull_item {
    int kf, n; const int* points; const uint8_t* octave; const uint8_t* close;        /* [n] x3 */
    int* n_mps; int* n_redundant; uint8_t* redundant;                                 /* outputs (host): [1], [1], [n] or NULL */
} sind_covis_cull_item;
int sind_covis_create(int cap_kf, int cap_feat, int cap_points, int nlevels, int max_queries, int device, sind_covis** out);
int sind_covis_destroy(sind_covis* c);
int sind_covis_clear(sind_covis* c);
int sind_covis_apply(sind_covis* c, const sind_covis_op* ops, int n);
int sind_covis_read_row(sind_covis* c, int kf, int* point, uint8_t* octave, uint8_t* stereo);          /* [cap_feat] x3 */
int sind_covis_read_points(sind_covis* c, const int* points, int n, int* n_obs, int* hist);           /* [n], [n], [n][nlevels] */
int sind_covis_count(sind_covis* c, const sind_covis_query* q, int Q);
int sind_covis_cull(sind_covis* c, const sind_covis_cull_item* items, int B, int th_obs);
typedef struct sindh_covis sindh_covis;
int sindh_covis_create(int cap_kf, int cap_feat, int cap_points, int nlevels, int max_queries, int device, sindh_covis** out);   /* max_queries and device are not used */
int sindh_covis_destroy(sindh_covis* c);
int sindh_covis_clear(sindh_covis* c);
int sindh_covis_apply(sindh_covis* c, const sind_covis_op* ops, int n);
int sindh_covis_read_row(sindh_covis* c, int kf, int* point, uint8_t* octave, uint8_t* stereo);
int sindh_covis_read_points(sindh_covis* c, const int* points, int n, int* n_obs, int* hist);
int sindh_covis_count(sindh_covis* c, const sind_covis_query* q, int Q);
int sindh_covis_cull(sindh_covis* c, const sind_covis_cull_item* items, int B, int th_obs);

/* ------------------------------------------------------------------------------------------------------------
 * Mapping consumer.  Replaces, for B key frames at once, the body of
 *   generatePointCloud(imgRGB, imgDepth, imgDepthLast, imgDynaMask, imgDynaMaskLast, imgLabel, poseRelative, Twc)
 *                                                                              octomap_pub/src/pubPointCloud.cc:471-668
 * stride-2 back-projection, re-projection depth-consistency vote per cluster (:556-607, vecOcclusion), cluster rejection
 * (vecOcclusion[i] * 9 <= 0.4 * countNonZero(imgLabel == i) keeps cluster i, :641-663) and pcl::transformPointCloud(.., Twc) (:665).
 * Images are dense [B][height][width] (bgr x3), host or device pointers (inputs_on_device); pose_relative / Twc: [B][16] row-major
 * doubles (Eigen::Matrix4d values).  points [B][cap] receives tempCloudOneFrame in the reference's order (cluster 0, then the kept
 * clusters 1..11, raster order inside a cluster; masked / out-of-range pixels are NaN points, the cloud is not dense), n_points [B];
 * occlusion / label_count / kept: [B][12], may be NULL.  The statistical outlier filter that follows in the ROS node (:291-296) is
 * sind_cloud_filter_outliers below; the octree insertion after it (:299-365, octomap's serial insertRay, integrateNodeColor and the walk over the occupied
 * leaves) is sind_occmap_* further down, which reads the UNFILTERED clouds where this call left them (sind_occmap_insert_generated).
 *
 * sind_cloud_filter_outliers replaces pcl::StatisticalOutlierRemoval (setMeanK(mean_k), setStddevMulThresh(stddev_mul), filter(*temp1); the reference uses 100
 * and 1.0) for B clouds at once.  The contract is restated from PCL 1.10's applyFilterIndices over KdTreeFLANN / flann::L2_Simple<float>; parity with a real PCL /
 * FLANN build is UNPINNED.  Per cloud (csrc/host/cloud_filter.hpp holds the arithmetic, one source for host and device):
 *   - a point is finite if x, y, z are; only finite points are neighbours; a non-finite point gets distance 0, is not counted in valid and is never removed;
 *   - squared distances are FP32, uncontracted (d = 0; d += dx*dx; d += dy*dy; d += dz*dz);
 *   - distances[i] = (float)(sum / mean_k), sum (FP64) of sqrt((double)d) over the mean_k + 1 smallest squared distances to the finite points (i itself
 *     included), ascending, the first dropped: a function of the multiset, so ties between neighbours cannot change a bit;
 *   - sum and sq_sum (FP64) run over all points in index order (sq_sum adds the FP32 product d * d); mean = sum / valid, variance = (sq_sum - sum * sum / valid) /
 *     (valid - 1.0), stddev = sqrt(variance), threshold = mean + stddev_mul * stddev, literally (a negative variance gives a NaN threshold and nothing is removed;
 *     a NaN in stddev or threshold is reported with the bits 0x7ff8000000000000, since its sign and payload are the processor's choice);
 *   - point i is removed iff distances[i] > threshold; the rest keeps its input order.
 *   The one deliberate divergence: with fewer than mean_k + 1 finite points the reference reads past its neighbour arrays; here the cloud comes back unchanged with
 *   degenerate = 1, valid = the finite count, mean = stddev = threshold = 0 and all distances 0.
 * points is [B][stride] with n_points[b] used (n_points is a host array; points is a device pointer if inputs_on_device); n_points[b] = 0 is legal.  points == NULL
 * means the clouds that the last sind_cloud_generate on this handle left on the device (B at most that call's B; n_points is not read): the reference's pair of calls
 * then costs one upload of images and one download of the filtered cloud.  Outputs are host arrays: out [B][out_cap] with n_out [B] (a cloud that keeps more than
 * out_cap points -> SIND_E_CAPACITY, n_out filled, as sind_cloud_generate does; out may be NULL to get the counts only), distances [B][stride] (may be NULL; with
 * points == NULL stride only lays out this array), stats [B] (may be NULL): n_ring and n_brute count the finite points answered by the grid search and by the
 * brute-force launch (0 in the host twin).  Limits: B <= max_batch, 1 <= mean_k <= 128, a finite stddev_mul (SIND_E_ARG otherwise); a cloud of more than
 * sind_cloud_max_points points -> SIND_E_CAPACITY.  The workspace is allocated on the handle at the first filter call and reused; sind_cloud_generate is not affected.
 * Ten launches and one memset whatever B, and two host waits: one for the counts, one for the copies sized by them.
 * sindh_cloud_filter_outliers is the host twin (libsind_host.so too): the same arithmetic, its own exact search, host arrays only, no handle.
 */
typedef struct sind_cloud sind_cloud;
typedef struct sind_cloud_point { float x, y, z; uint8_t b, g, r, a; } sind_cloud_point;       /* pcl::PointXYZRGB payload */
int sind_cloud_create(double fx, double fy, double cx, double cy, double depth_scale, int width, int height, int max_batch, int device, sind_cloud** out);
int sind_cloud_destroy(sind_cloud* c);
int sind_cloud_max_points(sind_cloud* c);                    /* ceil(width / 2) * ceil(height / 2) */
int sind_cloud_generate(sind_cloud* c, int B, const uint8_t* bgr, const uint16_t* depth, const uint16_t* depth_last, const uint8_t* dyna, const uint8_t* dyna_last,
                        const uint8_t* label, const double* pose_relative, const double* Twc, int inputs_on_device, sind_cloud_point* points, int cap, int* n_points,
                        int* occlusion, int* label_count, int* kept);
typedef struct sind_cloud_filter_stats { double mean, stddev, threshold; int valid, degenerate, n_ring, n_brute; } sind_cloud_filter_stats;
int sind_cloud_filter_outliers(sind_cloud* c, int B, const sind_cloud_point* points, int stride, const int* n_points, int inputs_on_device, int mean_k,
                               double stddev_mul, sind_cloud_point* out, int out_cap, int* n_out, float* distances, sind_cloud_filter_stats* stats);
int sind_cloud_filter_max_mean_k(void);                      /* the built maximum of mean_k: 128 */
int sindh_cloud_filter_outliers(int B, const sind_cloud_point* points, int stride, const int* n_points, int mean_k, double stddev_mul, sind_cloud_point* out,
                                int out_cap, int* n_out, float* distances, sind_cloud_filter_stats* stats);

/* ------------------------------------------------------------------------------------------------------------
 * Occupancy map of the mapping consumer (octomap_pub/src/pubPointCloud.cc:299-365): per key frame, octotree->insertRay(center, p) for every point of
 * tempCloudOneFrame with p.z >= 0 (:304-311), then integrateNodeColor for every point (:317-320), and the walk over the occupied leaves that becomes the published
 * cloud (:349-365).  A device-resident map on a handle of its own.  octomap is not available to this project and the reference does not vendor it: the contract below
 * is restated from octomap 1.9 AS RECALLED (ColorOcTree, OccupancyOcTreeBase::insertRay / updateNodeLogOdds, OcTreeBaseImpl::computeRayKeys).  PARITY WITH A REAL
 * OCTOMAP BUILD IS UNPINNED; the contract is what is built and tested.  csrc/host/occmap.hpp is the one source of the arithmetic for host and device.
 *
 * The map is FLAT: every voxel lives at octomap's finest depth (16); inner nodes and pruned leaves exist in the SNAPSHOT TREE taken from it (further down).  A voxel has a 3 x 16-bit key, known (0 / 1), logodds (FP32; 0 when it becomes known) and a
 * colour r, g, b (255, 255, 255 when it becomes known).
 * Create: resolution (the reference: 0.020; accepted range [1e-6, 1e6]), prob_hit 0.7, prob_miss 0.4, clamp_min 0.1192, clamp_max 0.971, occ_thres (octomap's
 *   default 0.5; the reference sets 0.7 at :119) -- each probability, inside (0, 1), becomes (float) log(p / (1 - p)), once, on the host, with the C library.
 *   resolution_factor = 1.0 / resolution.  max_voxels: the known voxels the map may hold; max_points: the largest cloud.  Both at most 2^26 (SIND_E_CAPACITY).
 * Keys: key(c) = (int) floor(resolution_factor * (double) c) + 32768 for a float coordinate c, valid iff 0 <= key < 65536;
 *   coord(k) = ((double) ((int) k - 32768) + 0.5) * resolution.
 * One ray = insertRay(origin, end), no max range, lazy_eval = false; origin and end are float triples:
 *   1. both keys; if either is invalid the ray does nothing and counts in n_skipped.  2. equal keys: the miss list is empty.
 *   3. otherwise computeRayKeys; the miss list starts with key(origin).  direction = end - origin per component in FP32; length = (float) sqrt(dx*dx + dy*dy + dz*dz)
 *      (the sum in FP32, left to right, uncontracted; the root correctly rounded); direction /= length in FP32.  Per axis: step = +1 / -1 / 0 by the sign of
 *      direction[i]; for step != 0, in FP64, border = coord(key[i]) + (double) (float) (step * resolution * 0.5), tMax = (border - (double) origin[i]) /
 *      (double) direction[i], tDelta = resolution / fabs((double) direction[i]); otherwise both DBL_MAX.  Loop: dim = tMax0 < tMax1 ? (tMax0 < tMax2 ? 0 : 2) :
 *      (tMax1 < tMax2 ? 1 : 2) (strict: a tie goes to the later axis); key[dim] += step[dim]; tMax[dim] += tDelta[dim]; stop if the key equals key(end); stop if
 *      min(tMax) > (double) length; otherwise append the key.
 *   4. every key of the miss list, in order, gets update(prob_miss_log); then key(end) gets update(prob_hit_log).
 *   5. update(u): an unknown voxel becomes known with 0 and (255, 255, 255); then v = v + u in FP32, clamped to [clamp_min_log, clamp_max_log].  (octomap's early
 *      return for a leaf already at the clamp changes no value and is not modelled.)
 * One key frame, points in index order: a point casts a ray iff x, y, z are finite and z >= 0.  After ALL rays of the key frame every point with finite x, y, z runs
 *   integrateNodeColor(x, y, z, r, g, b): an invalid key or an unknown voxel does nothing (the others count in n_coloured); a voxel whose colour is (255, 255, 255) is
 *   "not set" and takes (r, g, b); otherwise each channel becomes (uint8_t) ((double) prev * p + (double) new * (0.99 - p)), p = 1. - (1. / (1. + exp((double)
 *   logodds))), exp being the fdlibm restatement of csrc/host/fd_exp.hpp on both sides.  A white point therefore leaves the voxel "not set": the reference's behaviour.
 * ORDER: the clamp makes a voxel's value depend on the order of its hits and misses.  Rays act in point index order; a ray touches a voxel at most once; colours blend in
 *   point index order after the rays; B key frames in one call equal B calls in order (key frame b's colours see the log-odds after its rays and before those of b + 1).
 * Queries: occupied = every known voxel with logodds >= occ_thres_log as a sind_cloud_point (x, y, z = (float) coord(key), its colour, a = 0), in octomap's
 *   leaf_iterator order: ascending Morton code of the key from bit 15 down, z the most significant bit of each triple, then y, then x (the sort runs on the host).  out
 *   may be NULL to get the count; more than cap: SIND_E_CAPACITY with *n_out filled.  read: for n keys [n][3] the known flag, the log-odds bits and r, g, b [n][3]
 *   (zeros for an unknown voxel).  size: the number of known voxels (NOT octomap's size(), which counts inner nodes: that is n_nodes of the snapshot tree).  clear.
 * Capacity: a key frame that would take the map beyond max_voxels known voxels returns SIND_E_CAPACITY and leaves every value, colour and known flag as they were; in
 *   a batch the key frames before it are in the map (as B calls would leave it), it and the later ones are not, and their stats are zero.  The table has 2 max_voxels
 *   slots or more and refuses claims beyond three quarters of them; slots claimed by a refused key frame stay claimed (and unknown) until clear, so after refused
 *   key frames that claimed more than max_voxels / 2 slots in all, a key frame that fits may be refused too.  A cloud of more than max_points points: SIND_E_CAPACITY.
 * DELIBERATE DIVERGENCES from the reference's octomap:
 *   1. Non-finite points.  The reference feeds them to (int) floor(..), which is undefined; here they are skipped (no ray, no colour, not counted).  A non-finite origin
 *      is SIND_E_ARG.  Likewise a ray whose FP32 length underflows to 0 never ends in octomap's loop; here a key that would leave [0, 65536) ends it.
 *   2. The map itself is never pruned.  octomap merges eight sibling leaves of equal value and colour into their parent WHILE IT INSERTS.  Log-odds are unaffected (a
 *      pruned leaf equals its children and is expanded by copying before any update).  Two things differ: occupied reports the 8^k finest voxels where the reference
 *      reports one coarser leaf centre (the snapshot tree below reports the coarser leaf), and an integrateNodeColor that meets a pruned leaf colours all of that
 *      leaf's voxels at once (tests/occmap_ref.py carries a pruning tree that counts these; profiles/occmap.txt has the count on real data).  Inner nodes, prune(),
 *      the .ot file and fullMapToMsg's data come from the SNAPSHOT TREE, which is the fully pruned form of the flat map: it differs from the reference's online tree
 *      exactly where the flat map already differs (voxels coloured while they sat in a pruned leaf), and beyond that in inner-node colours that octomap keeps from a
 *      prune / expand history, which are white here.  (On the CPU, with the pruning tree of tests/occmap_ref.py as the online tree: where no colour met a pruned
 *      leaf the online tree's leaves equal the snapshot's, even without a final prune(); where one did, they do not: tests/test_occmap_tree_cpu.py.)
 * sind_occmap_insert: points [B][stride] with n_points[b] used (a host array; points is a device pointer if inputs_on_device), origins [B][3] floats (host);
 *   stats [B] (may be NULL).  sind_occmap_insert_generated reads the clouds that the last sind_cloud_generate on `cloud` left on the device (the reference inserts the
 *   UNFILTERED tempCloudOneFrame, so it does not chain on the filter); SIND_E_STATE if B exceeds that call's B.  Eleven launches per key frame whatever the cloud, on
 *   the handle's stream, ONE host wait per call, no allocation per call (the workspace lives on the handle; stats grows once if B > 8).
 * sindh_occmap_* are the host twin (libsind_host.so too): the literal sequential loops over a flat hash map, the same arithmetic, host arrays only.
 *
 * SNAPSHOT TREE (sind_occmap_tree, sind_occmap_write_ot): octomap's tree over the flat map as it is at the call -- what octotree->write(".ot") (:184) saves,
 * what octomap_msgs::fullMapToMsg (:327-340) publishes and what the leaf loop (:349-365) walks.  Read-only on the map; insert, occupied, read, size and clear are as
 * before.  Restated from octomap 1.9 AS RECALLED (OcTreeBaseImpl::prune / pruneNode / isNodeCollapsible, OccupancyOcTreeBase::updateInnerOccupancy,
 * ColorOcTree::getAverageChildColor, OcTreeBaseImpl::writeData, AbstractOcTree::write); PARITY WITH A REAL OCTOMAP BUILD, and with its file format, IS UNPINNED.
 * csrc/host/occmap_tree.hpp is the one source of the arithmetic for host and device.
 * Tree: depth 16.  The child index at depth d (0 .. 15) of a key is ((kz >> (15-d)) & 1) << 2 | ((ky >> (15-d)) & 1) << 1 | ((kx >> (15-d)) & 1), the Morton order of
 *   occupied.  Every known voxel is a depth-16 leaf, every proper prefix of a known key an inner node.  An empty map is an empty tree: 0 nodes, no root.
 * Inner value: the maximum log-odds of the existing children (updateOccupancyChildren), compared as floats.
 * Inner colour: inner_colour = 0: (255, 255, 255), which is what the reference's tree holds (its updateInnerOccupancy() call is commented out, :321).
 *   inner_colour = 1: getAverageChildColor, bottom-up: per channel the integer sum over the existing children whose colour is not (255, 255, 255), integer-divided by
 *   their number; white if there is none; an inner child contributes its own average.
 * Pruning (prune = 1, OcTreeBaseImpl::prune()): for depth 15 down to 1 (the root is never pruned) every node of that depth that is collapsible -- all eight children
 *   exist, none has children, all eight are equal in value (float ==) and colour -- becomes a leaf with child 0's value and colour; a depth that prunes nothing ends
 *   the walk.  On a tree that starts flat ONE BOTTOM-UP SWEEP OVER THE LEVELS GIVES THE SAME RESULT (a node can only become collapsible through children that
 *   collapsed one level below, and below a level that pruned nothing no level can prune): the device does the sweep, the host twin the literal loop.  prune = 0 keeps
 *   every depth-16 leaf.  Pruning and inner_colour commute (eight equal children average and maximise to themselves).
 * Stream (writeData): the nodes in pre-order, 8 bytes each: the FP32 value, r, g, b, then one byte with bit i set iff child i exists (0 for a leaf); the children
 *   follow in ascending i.  8 n_nodes bytes.
 * .ot file (sind_occmap_write_ot): the lines "# Octomap OcTree file", "# (feel free to add / change comments, but leave the first line as it is!)", "#",
 *   "id ColorOcTree", "size <n_nodes>", "res <resolution, as a default-precision C++ ostream prints it>", "data", each ended by '\n'; then the stream.  fullMapToMsg is
 *   {id: "ColorOcTree", resolution, binary: false, data: the stream}.
 * Leaves: in pre-order, which is leaf_iterator order: a sind_cloud_point (the centre, the colour, a = 0) and the depth.  The centre per axis of a leaf of depth d that
 *   holds the key k is (float) (((double) ((int) (k >> (16-d) << (16-d)) - 32768) + 0.5 * (double) (1 << (16-d))) * resolution).  occupied_only = 1 keeps the leaves
 *   with value >= occ_thres_log: with prune = 1 the list the reference's loop walks, with prune = 0 the list of sind_occmap_occupied, byte for byte.
 * Stats: n_nodes (octomap's size()), n_inner, n_leaves, n_pruned (nodes collapsed), n_occupied_leaves, leaves_at_depth[17]; they do not depend on occupied_only.
 * Call: data (cap_bytes), leaves / leaf_depth (cap_leaves) and n_leaves_out may each be NULL (leaf_depth only together with leaves); with no outputs the call returns
 *   the counts: stats, and in *n_leaves_out the leaves the list would hold.  8 n_nodes > cap_bytes or more leaves than cap_leaves: SIND_E_CAPACITY with the counts
 *   filled and no output written, as sind_occmap_occupied does.  The call never changes the map and keeps nothing between calls.
 * Workspace and limit: the table of inner nodes is allocated at the first tree call and kept on the handle: as many slots as the flat table has (the power of two >=
 *   max(1024, 2 max_voxels)), 64 bytes each, and A TREE MAY HAVE HALF AS MANY INNER NODES AS THERE ARE SLOTS (so at least max_voxels, and at least 512); a map whose
 *   tree needs more (N scattered voxels can need 16 N) returns SIND_E_CAPACITY, without counts.  The output staging grows to the largest tree asked for.
 * Device schedule: 18 launches bottom-up (a sweep that resets the table, the voxels, one kernel per depth 15 .. 0) and, if any output is asked for, 16 top-down (one per
 *   depth), on the handle's stream, whatever the map; TWO host waits per call (the counts, then the copies sized by them), one if no output is asked for.
 *   sind_occmap_write_ot does the same and then writes the file on the host.
 */
#define SIND_OCCMAP_MIN_RESOLUTION 1e-6
#define SIND_OCCMAP_MAX_RESOLUTION 1e6
typedef struct sind_occmap sind_occmap;
typedef struct sind_occmap_stats { int n_rays, n_skipped, n_coloured, n_miss_updates, n_new_voxels; } sind_occmap_stats;
int sind_occmap_create(double resolution, double prob_hit, double prob_miss, double clamp_min, double clamp_max, double occ_thres, int max_voxels, int max_points,
                       int device, sind_occmap** out);
int sind_occmap_destroy(sind_occmap* h);
int sind_occmap_clear(sind_occmap* h);
int sind_occmap_size(sind_occmap* h);                        /* >= 0: the known voxels; octomap's size() is sind_occmap_tree's n_nodes */
int sind_occmap_insert(sind_occmap* h, int B, const sind_cloud_point* points, int stride, const int* n_points, const float* origins, int inputs_on_device,
                       sind_occmap_stats* stats);
int sind_occmap_insert_generated(sind_occmap* h, sind_cloud* cloud, int B, const float* origins, sind_occmap_stats* stats);
int sind_occmap_occupied(sind_occmap* h, sind_cloud_point* out, int cap, int* n_out);
int sind_occmap_read(sind_occmap* h, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb);
typedef struct sindh_occmap sindh_occmap;
int sindh_occmap_create(double resolution, double prob_hit, double prob_miss, double clamp_min, double clamp_max, double occ_thres, int max_voxels, int max_points,
                        sindh_occmap** out);
int sindh_occmap_destroy(sindh_occmap* h);
int sindh_occmap_clear(sindh_occmap* h);
int sindh_occmap_size(sindh_occmap* h);
int sindh_occmap_insert(sindh_occmap* h, int B, const sind_cloud_point* points, int stride, const int* n_points, const float* origins, sind_occmap_stats* stats);
int sindh_occmap_occupied(sindh_occmap* h, sind_cloud_point* out, int cap, int* n_out);
int sindh_occmap_read(sindh_occmap* h, const uint16_t* keys, int n, uint8_t* known, uint32_t* logodds, uint8_t* rgb);

/* The snapshot tree (contract above, "SNAPSHOT TREE"). */
typedef struct sind_occmap_tree_stats { int n_nodes, n_inner, n_leaves, n_pruned, n_occupied_leaves; int leaves_at_depth[17]; } sind_occmap_tree_stats;
int sind_occmap_tree(sind_occmap* h, int prune, int inner_colour, int occupied_only,
                     uint8_t* data, size_t cap_bytes,                                                      /* the writeData stream; may be NULL */
                     sind_cloud_point* leaves, uint8_t* leaf_depth, int cap_leaves, int* n_leaves_out,     /* each may be NULL (leaf_depth only with leaves) */
                     sind_occmap_tree_stats* stats);
int sind_occmap_write_ot(sind_occmap* h, int prune, int inner_colour, const char* path);                   /* the .ot file: header + stream */
int sindh_occmap_tree(sindh_occmap* h, int prune, int inner_colour, int occupied_only, uint8_t* data, size_t cap_bytes, sind_cloud_point* leaves, uint8_t* leaf_depth,
                      int cap_leaves, int* n_leaves_out, sind_occmap_tree_stats* stats);
int sindh_occmap_write_ot(sindh_occmap* h, int prune, int inner_colour, const char* path);

/* helper of the rgbd_tum_noros-shaped harness (sindslam_amd/harness.py): PNG scanline reconstruction, raw = h x (1 + stride) bytes */
int sind_png_unfilter(const uint8_t* raw, int h, int stride, int bytes_per_pixel, uint8_t* out);

/* ------------------------------------------------------------------------------------------------------------
 * One long sequence, sharded by frame, with results EQUAL to the sequential loop (rgbd_tum_noros.cc:110-170 is the loop it equals).
 * The sequence is cut into world x streams contiguous lock-step chunks, one per pipeline stream; chunk 0 starts like the reference loop, a later chunk starts `warmup`
 * frames early from an empty state (speculation).  After the lock-step steps every chunk seam is VERIFIED by comparing 128-bit fingerprints of the inter-frame state
 * (DynaDetect.h:165-178, rolled at DynaDetect.cc:1660-1664) and a chunk whose rebuilt state is not its predecessor's true end state is REPAIRED: the stateful tails of
 * its first frames run again from the true state (on the retained phase-A outputs, then as whole frames on a small second pipeline) until the states agree.  Between
 * ranks a round costs one all-gather of 32 bytes per chunk and, for a mismatching seam between two ranks, one send / receive of the state blob -- over RCCL
 * (sind_seq_net_rccl on a sind_comm) or TCP (sind_seq_net_tcp: ranks without a communicator between them, several ranks rehearsed on one card).
 * Everything below is C++ inside the library (csrc/host/seq.cpp): a C++ caller needs neither Python nor torch.distributed for the exact sharded mode.
 *
 * Positions: position q = frame q + 1 of the sequence (frame 0 only primes, like the reference's first frame).  Outputs are caller arrays indexed by FRAME. */
typedef struct sind_seq sind_seq;
typedef struct sind_seq_net sind_seq_net;
typedef struct sind_seq_config {
    sind_pipe_config pipe;          /* streams = chunks PER RANK; frames_per_step is set by the plan (ignored on input) */
    long long frames;               /* positions of the job = sequence length - 1 */
    int steps;                      /* > 0: exactly this many lock-step steps (bench.py); 0: as many as frames_per_step asks for */
    int frames_per_step;            /* steps == 0: a step holds at most this many frames per chunk */
    int warmup;                     /* frames a chunk after the first starts early to rebuild the inter-frame state */
    int repair_streams, repair_frames_per_step;     /* the repair pipeline (0 = min(streams, 8) x 4) */
    int retain_frames;              /* steps holding the first n owned frames of the later chunks keep their phase-A outputs for replays; -1 = every step, 0 = none */
    int verify;                     /* 0: keep the speculative results (valid masks, not identical behind some seams) */
} sind_seq_config;
/* source callbacks: device pointers of the `count` frames at these positions, laid out [count][H][W][3] / [count][H][W] (valid until the next call), and the HOST bgr
 * frame of one position (priming); return 0 */
typedef int (*sind_seq_batch_fn)(void* user, const long long* positions, int count, const uint8_t** bgr_dev, const uint16_t** depth_dev);
typedef int (*sind_seq_frame_fn)(void* user, long long position, const uint8_t** bgr_host);
typedef int (*sind_seq_hook_fn)(void* user, int index);       /* step hook: the owned frames of step `index` are out; round hook: repair round `index` has ended (called on every rank) */
int sind_seq_net_tcp(int rank, int world, const char* host_or_null /* 127.0.0.1 */, int base_port, sind_seq_net** out);      /* rank r listens on base_port + r */
int sind_seq_net_rccl(sind_comm* c, sind_seq_net** out);
int sind_seq_net_destroy(sind_seq_net* n);
int sind_seq_create(const sind_seq_config* cfg, sind_seq_net* net_or_null /* one rank */, sind_seq** out);
int sind_seq_destroy(sind_seq* q);
int sind_seq_plan(sind_seq* q, int* frames_per_step, int* steps, int* n_chunks, long long* first_last_start /* n_chunks x 3, or NULL */);
int sind_seq_set_host_source(sind_seq* q, const uint8_t* bgr, const uint16_t* depth, long long n_frames);      /* the whole sequence in host memory: [n][H][W][3] u8, [n][H][W] u16 */
int sind_seq_set_source(sind_seq* q, sind_seq_batch_fn batch, sind_seq_frame_fn frame, void* user);
/* sink: arrays of n_frames entries indexed by frame (dyna / label / mask [n][H][W]; kps [n][cap], nkp [n], desc [n][cap][32]); any may be NULL; a rank fills the frames it owns */
int sind_seq_set_outputs(sind_seq* q, long long n_frames, uint8_t* dyna, uint8_t* label, uint8_t* mask_dilated, sind_keypoint* kps, int cap, int* nkp, uint8_t* desc);
int sind_seq_set_hooks(sind_seq* q, sind_seq_hook_fn step_hook, sind_seq_hook_fn round_hook, void* user);
int sind_seq_prime(sind_seq* q);
int sind_seq_warm(sind_seq* q, int steps);        /* untimed rehearsal after sind_seq_prime: the first `steps` steps synchronously + one step of the repair pipeline; call sind_seq_prime again */
int sind_seq_set_emit_main(sind_seq* q, int on);  /* 0: the frames of a lock-step step are not copied to the sink (the step hook reads sind_seq_step_outputs itself); repaired frames always are */
int sind_seq_submit(sind_seq* q, int step);       /* steps 0 .. steps - 1 in order; software-pipelined: the results of step - 1 are delivered */
int sind_seq_flush(sind_seq* q);                  /* delivers the last step */
int sind_seq_verify(sind_seq* q);                 /* seam verification and repairs (collective over the ranks) */
int sind_seq_run(sind_seq* q);                    /* prime + every step + flush + verify */
/* seams, mismatched seams, rounds, runners, repaired chunks, repair frames, repair steps, overridden frames, runners to chunk end, max frames to converge, replay frames,
 * replay calls, runners past replay, retained steps dropped, repair seconds, flush seconds */
int sind_seq_stats(sind_seq* q, double out16[16]);
sind_pipe* sind_seq_pipeline(sind_seq* q);        /* the main pipeline of this rank (sind_pipe_stats, sind_pipe_gather_masks, ...) */
int sind_seq_step_outputs(sind_seq* q, const uint8_t** dyna, const uint8_t** label, const uint8_t** mask_dilated);   /* the page-locked [S][T][H][W] arrays of the last delivered step */

/* ---- SegAndMerge piece extraction on the device: parity-test access to its border following (k_piece_contours) -------------------------------------------------------
 * n bit planes (host, [n][height][ceil(width / 64)] words, bit x & 63 of word x / 64) -> their external borders from the device (one launch, one wave per plane) and from
 * the host function (find_contours, external only).  Per plane: counts [3] = contours, points, status (0; 1 = more than cap_contours contours; 2 = more than cap_points
 * chain points: the device then stops and reports what it had, the host reports the totals and fills what fits); hdr [cap_contours][10] = start x, start y, length,
 * offset of the first point, box x0 y0 x1 y1, twice the contour area (low word, high word); pts [cap_points][2] = x, y of every point, contour after contour. */
int sind_debug_contours(const unsigned long long* planes, int n, int width, int height, int device, int cap_contours, int cap_points,
                        int* counts_gpu, int* hdr_gpu, int* pts_gpu, int* counts_host, int* hdr_host, int* pts_host);
/* The whole stage (reference DynaDetect.cc:664-729 and the ranking :733-752): n frames of k cluster planes [n][k][words] (all k are cut), occ1 and labelForSegEdge (already
 * dilated) [n][words], depth [n][height][width] u16 -> the pieces from the device stage (one batched object of capacity n: 13 launches whatever the frames hold) and from the
 * host function; ONE frame (n = 1; width a multiple of 64, height of 8) instead runs through a tail of its own with the switch on: its capacity-1 stage on its own stream,
 * the fallback to the host function, the ranking and k_piece_commit (planes and piece_of then come from the device).  Per frame and side: info [4] = number of pieces C,
 * status (0; else a plane exceeded a capacity: batched, the device results are not to be used; one frame, the tail fell back and the results are the host function's), and for one
 * frame the tail's counters frames_on_device, frames_fallen_back (0 otherwise);
 * the first min(C, cap) pieces in discovery order: recs [cap][12] = cluster, start x, start y, contour length, twice the contour area (low, high word), hasLianjie, box
 * x0 y0 x1 y1, rank after the host's sort (-1 when C is 0 or above 254); vals [cap][2] = area, cz; piece and connection planes [cap][words]; piece_of [height * width] =
 * rank of the piece that owns the pixel, C + 1 elsewhere (untouched when nothing is ranked).  The sort and piece_of are the host's on both sides. */
int sind_debug_seg_pieces(const unsigned long long* planes, int k, const unsigned long long* occ1, const unsigned long long* label_edge, const uint16_t* depth, int n, int width, int height,
                          float depth_scale, int device, int cap, int* info_gpu, int* recs_gpu, float* vals_gpu, unsigned long long* pieces_gpu, unsigned long long* conn_gpu, uint8_t* piece_of_gpu,
                          int* info_host, int* recs_host, float* vals_host, unsigned long long* pieces_host, unsigned long long* conn_host, uint8_t* piece_of_host);
/* The piece stage batched per round (PieceBatch, csrc/dyna.hpp): n frames (1..64; width a multiple of 64, height of 8) of k cluster planes, occ1, labelForSegEdge, depth as
 * above, plus occ2 and the 8-bit normalised depth [n][height][width] u8 for the region-adjacency statistics.  Device side (the *_gpu outputs): the real PieceBatch in chunks
 * of `chunk` frames (n = 5, chunk 3: a full and a partial chunk) with the depth planes at non-uniform device offsets (the stage's depth table), the host step
 * (seg_pieces_order), k_piece_commit_frames / k_piece_paint_frames into a RagBatch's device slab and launch_rag_frames on it; a frame whose status is not 0 runs the host
 * function and is packed from the host into the same run.  Host side: the host function, the ranking, rag_pack and launch_rag_frames on a host-packed slab (the path of a
 * round without the switch).  Per frame and side: info [4] = number of pieces C, error code (0, or SIND_E_CAPACITY for more than 254 pieces: nothing else is returned for
 * the frame and sind_last_error holds the text), fell back (a capacity of the device stage was exceeded), committed on the device; recs / vals / piece and connection planes /
 * piece_of in the layout of sind_debug_seg_pieces (on the device side the planes and piece_of are read back from where the kernels wrote them: the slab's [0, C) / [C, 2C)
 * sets in rank order, zeros of a missing connection area included); rag [rag_cap] ints = the frame's result block (3 C^2 + C + 256 C ints: overlap, overlapPlane,
 * connection overlap, connection areas, histograms). */
int sind_debug_pieces_batch(const unsigned long long* planes, int k, const unsigned long long* occ1, const unsigned long long* label_edge, const uint16_t* depth, const uint8_t* occ2,
                            const uint8_t* depth_n, int n, int width, int height, float depth_scale, int device, int chunk, int cap, int rag_cap,
                            int* info_gpu, int* recs_gpu, float* vals_gpu, unsigned long long* pieces_gpu, unsigned long long* conn_gpu, uint8_t* piece_of_gpu, int* rag_gpu,
                            int* info_host, int* recs_host, float* vals_host, unsigned long long* pieces_host, unsigned long long* conn_host, uint8_t* piece_of_host, int* rag_host);
/* The round's switch (default off; with it off nothing is launched, allocated or changed): in the non-split `rounds` schedule with the batched RAG stage on, a round's
 * frames cut their pieces through their k-means group's PieceBatch -- one chain of 13 launches per chunk of rag_chunk (at most 64) frames instead of the host function,
 * the planes committed straight into the RAG batch's device slab: two waits per chunk, none per frame, no piece plane over PCIe in either direction.  Every other
 * schedule (chains, flow_chains, two_chains, split_rounds, rounds without the batched RAG stage) is untouched: there sind_pipe_set_device_pieces alone decides, and
 * sind_pipe_device_pieces keeps counting only that per-tail stage.  The workspaces (about 2 GB per k-means group at 640 x 480 and chunk 32, csrc/dyna.hpp) are made by the
 * first round that uses them; an allocation failure fails the step with its text.  frames_batched: frames whose pieces were cut and committed on the device;
 * frames_fallback: frames that exceeded a capacity of the stage and ran the host function.  A frame with no cluster to cut, no pieces, or more than 254 (SIND_E_CAPACITY, as
 * on every path) counts as neither.  Same results, bit for bit.  Not while a step is pending. */
int sind_pipe_set_pieces_batch(sind_pipe* p, int on);
int sind_pipe_get_pieces_batch(sind_pipe* p, int* on, long long* frames_batched, long long* frames_fallback);
/* The switch: SegAndMerge's piece extraction of a handle on the GPU instead of the host.  Off by default; the results do not depend on it.  A frame in which a plane
 * exceeds a capacity of the device stage runs the host function and is counted as fallen back.  The second call of each pair only reads. */
int sind_dyna_set_device_pieces(sind_dyna* d, int on);
int sind_dyna_device_pieces(sind_dyna* d, int* on, long long* frames_on_device, long long* frames_fallen_back);
int sind_pipe_set_device_pieces(sind_pipe* p, int on);      /* every stream's tail; not while a step is pending */
int sind_pipe_device_pieces(sind_pipe* p, int* on, long long* frames_on_device, long long* frames_fallen_back);

#ifdef __cplusplus
}
#endif
#endif
