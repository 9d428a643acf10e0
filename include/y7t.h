/*
 * y7t.h -- C ABI of liby7t.so, the MI355X (gfx950) implementation of the Yolov7-tracker hot path.
 *
 * The reference (JackWoo0831/Yolov7-tracker) is pure Python and has no FFI of its own; its
 * "operator API" for this path is the set of Python call sites cited on each function below
 * (paths relative to the reference repo).  This header is what a binding for those call sites
 * binds; INTEGRATION.md shows the ctypes stubs a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is caller-owned; pointers are DEVICE pointers unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous
 *     with respect to the host unless stated otherwise;
 *   - return value: 0 = OK, < 0 = error (message via y7t_last_error(), thread-local);
 *   - no torch types, no exceptions across the boundary, no hidden global state except the
 *     explicit id counter object that mirrors BaseTrack._count.
 */
#ifndef Y7T_H
#define Y7T_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* y7t_stream;

enum { Y7T_OK = 0, Y7T_E_ARG = -1, Y7T_E_HIP = -2, Y7T_E_CAPACITY = -3, Y7T_E_STATE = -4 };

/* Kalman filter kinds == KALMAN_DICT keys, tracker/basetrack.py:64-69 */
enum { Y7T_KALMAN_DEFAULT = 0, Y7T_KALMAN_NAIVE = 1, Y7T_KALMAN_BOTSORT = 2, Y7T_KALMAN_STRONGSORT = 3 };
/* tracker kinds == TRACKER_DICT keys implemented on the device, tracker/track.py:56-65 */
enum { Y7T_TRACKER_SORT = 0, Y7T_TRACKER_BYTETRACK = 1, Y7T_TRACKER_BOTSORT = 2, Y7T_TRACKER_DEEPSORT = 3, Y7T_TRACKER_C_BIOU = 4,
       Y7T_TRACKER_UAVMOT = 5, Y7T_TRACKER_STRONGSORT = 6, Y7T_TRACKER_DEEPMOT = 7 };
#define Y7T_TRACKER_BOTSORT_REID 8      /* BoT-SORT with its appearance branch: a kind of y7t_tracker_init beside the reference's eight tracker names (see below) */

const char* y7t_last_error(void);
int y7t_version(void);
/* diagnostics: name of the kernel variant the last launch made by this thread selected, e.g. "patch<16,16,128>", "igemm<128,128,32,2> 1x1",
 * "patch_strip<40,128>" (the conv dispatch rules -- tile shape, LDS-patch vs generic, split-K -- live inside the library and depend on
 * the batch size; tests and bench.py read the launch list of a plan back through y7t_det_forward_ops(i, i+1) + this) */
const char* y7t_last_kernel(void);
/* number of HIP devices visible (0 when there is none); host-synchronous */
int y7t_device_count(void);
/* A HIP stream restricted to a set of compute units (bit i of mask_words_host = CU i; hipExtStreamCreateWithCUMask).  The reference runs the detector
 * and `tracker.update` one after the other on one stream (tracker/track.py:144-151); the pipelined form of that loop (bench.py, track.py --batch)
 * runs the tracker's single-workgroup frame steps beside the next batch's convolutions, and gives them compute units of their own so that they do
 * not queue behind / share issue slots with 256-thread convolution workgroups.  The stream is an ordinary hipStream_t for every other call here. */
int y7t_stream_create_cu_mask(const uint32_t* mask_words_host, int n_words, y7t_stream* out_stream_host);
int y7t_stream_destroy(y7t_stream stream);

/* ---------------------------------------------------------------- tracker math (float64) ---- */

/* matching.iou_distance -> ious -> cython_bbox.bbox_overlaps, tracker/matching.py:44-82.
 * cost[i*m + j] = 1 - IoU(a_i, b_j) with the "+1 pixel" convention. a: n x 4 tlbr, b: m x 4. */
int y7t_iou_cost_f64(const double* a_tlbr, int n, const double* b_tlbr, int m, double* cost, y7t_stream stream);
/* matching.structure_similarity_distance (tracker/matching.py:284-388, UAVMOT): out[n x m] = max(0, cosine distance) of the structure vectors
 * [max, min, included angle] of n track centres (mean[0:2], float64 arithmetic) and m detection centres (get_xy(): float32 values, float32 distance
 * arithmetic).  Device pointers; n + m <= 2048 (one workgroup holds the vectors). */
int y7t_structure_distance_f64(const double* track_xy, int n, const double* det_xy, int m, double* out, y7t_stream stream);

/* KalmanFilter.initiate, tracker/kalman_filter.py:190-221 (xyah), :436-467 (xywh).
 * z: K x 4 measurements; mean: K x 8; cov: K x 64.  flags bit0: keep the std products in
 * float32 (what the reference does under numpy >= 2 when handed a float32 measurement). */
int y7t_kf_initiate_f64(int kind, const double* z, double* mean, double* cov, int K, int flags, y7t_stream stream);

/* KalmanFilter.multi_predict, tracker/kalman_filter.py:289-329, fused with the "zero the last
 * state component of non-Tracked tracks" step of STrack.multi_predict, tracker/basetrack.py:253-271.
 * In place on mean (N x 8) / cov (N x 64); zero_last_mask: N bytes or NULL. */
int y7t_kf_multi_predict_f64(int kind, double* mean, double* cov, const uint8_t* zero_last_mask, int N,
                             y7t_stream stream);

/* KalmanFilter.project, tracker/kalman_filter.py:260-287 (conf: N confidences for the NSA filter or NULL).
 * pmean: N x 4, pcov: N x 16. */
int y7t_kf_project_f64(int kind, const double* mean, const double* cov, const double* conf, double* pmean,
                       double* pcov, int N, y7t_stream stream);

/* KalmanFilter.update, tracker/kalman_filter.py:331-363, batched over K (track, measurement) pairs:
 * pair k updates track track_idx[k] (or track k when track_idx is NULL) with z[k] (K x 4). In place. */
int y7t_kf_update_batch_f64(int kind, double* mean, double* cov, const double* z, const int* track_idx,
                            const double* conf, int K, y7t_stream stream);

/* KalmanFilter.gating_distance(metric='maha'), tracker/kalman_filter.py:365-411:
 * out[i*M + j] = squared Mahalanobis distance of measurement j to track i. */
int y7t_kf_gating_f64(int kind, const double* mean, const double* cov, const double* z, int N, int M,
                      int only_position, double* out, y7t_stream stream);

/* matching.linear_assignment -> lap.lapjv(cost, extend_cost=True, cost_limit=limit),
 * tracker/matching.py:30-41.  cost: n x m row-major.  x[n]: column of row i or -1; y[m]: row of
 * column j or -1; opt (may be NULL): sum of the kept costs.  One workgroup on the device;
 * workspace: y7t_lapjv_workspace_bytes(n, m) bytes of device memory. */
size_t y7t_lapjv_workspace_bytes(int n, int m);
int y7t_lapjv_f64(const double* cost, int n, int m, double cost_limit, int* x, int* y, double* opt, void* workspace,
                  y7t_stream stream);
/* The same with HOST pointers (SURVEY 8b "+ _host variant": matching.linear_assignment is called with numpy arrays): cost / x / y / opt live in host
 * memory; the library stages them through device buffers it owns (grown on demand), solves on the device and returns when x / y / opt are written.
 * No CPU solver behind it: without a GPU it fails like every other entry point.  Not re-entrant (one staging allocation per process). */
int y7t_lapjv_f64_host(const double* cost_host, int n, int m, double cost_limit, int* x_host, int* y_host, double* opt_host, y7t_stream stream);
/* Diagnostics: how many assignments of this process met a tie (a pair exactly at cost_limit, equal-cost alternatives in a small problem) and were
 * re-solved with lap's lapjv.cpp run literally, because the optimum lapjv returns is then a property of its own scan order (matching.py:30-44). */
int y7t_lap_literal_calls(void);

/* ---------------------------------------------------------------- device-resident tracker ---- */
/* BaseTrack._count (tracker/basetrack.py:22,43-46): one int in device memory, shared by every
 * tracker object of the process.  The caller allocates 4 bytes and zeroes them. */

/* size in bytes of the state blob of one tracker (tracked_stracks + lost_stracks pool etc.) */
size_t y7t_tracker_state_bytes(int cap_tracks, int cap_dets);

/* BaseTracker.__init__ / ByteTrack.__init__, tracker/basetrack.py:346-367, tracker/bytetrack.py:9-17.
 * conf_thresh = opts.conf_thresh, iou_thresh = opts.iou_thresh, max_time_lost = int(frame_rate/30*track_buffer).
 * flags bit0: numpy>=2 float32 flow of freshly initiated tracks (see y7t_kf_initiate_f64). */
int y7t_tracker_init(void* state, size_t state_bytes, int tracker_kind, int kalman_kind, int cap_tracks, int cap_dets,
                     double conf_thresh, double iou_thresh, int max_time_lost, int flags, int* id_counter,
                     y7t_stream stream);

/* the end of a tracker object's life (the reference: garbage collection of the BaseTracker instance, tracker/track.py:132 creates one per sequence): call before
 * freeing or re-purposing `state`; the library forgets the host-side notes it keeps per initialised blob (tracker kind, LDS arena size) */
int y7t_tracker_release(void* state);

/* ByteTrack.update / BaseTracker.update (tracker/bytetrack.py:41-204, tracker/basetrack.py:368-487) as ONE
 * kernel launch, one workgroup per tracker.  `batch` trackers step together (independent sequences):
 *   states[b]   state blob of tracker b
 *   dets[b]     n x 6 float32 rows [x1,y1,x2,y2,conf,cls] (what post_process_v7 hands over, track.py:234-244)
 *   n_dets[b]   row count, read ON THE DEVICE (so it can come straight from NMS); < 0 = update_without_detection
 *   out_rows[b] out_cap x 8 float64 rows (track_id, x, y, w, h, cls, score, slot) of the returned tracks
 *   out_count[b] number of returned tracks
 * states/dets/n_dets/out_rows/out_count (and gmc_warps, may be NULL) are DEVICE arrays of `batch` entries. threads: 0 = default. */
int y7t_tracker_step_batch(void* const* states, const float* const* dets, const int* n_dets, double* const* out_rows,
                           int* out_count, int out_cap, int batch, int threads, const double* const* gmc_warps,
                           y7t_stream stream);

/* n_frames CONSECUTIVE frames of one tracker in one launch (the per-frame loop of tracker/track.py:138-179 for a caller that already holds a batch's
 * detections, e.g. `--batch N`): frame f = dets[f] / n_dets[f] (read on the device) -> out_rows[f], *out_count[f]; all five are DEVICE arrays of
 * n_frames entries (gmc_warps may be NULL).  Exactly the frames y7t_tracker_step would produce one by one. */
int y7t_tracker_step_frames(void* state, const float* const* dets, const int* n_dets, double* const* out_rows, int* const* out_count, int out_cap,
                            int n_frames, int threads, const double* const* gmc_warps, y7t_stream stream);

/* convenience for batch == 1 with host-known n (n < 0: update_without_detection, basetrack.py:489-537) */
int y7t_tracker_step(void* state, const float* dets, int n, double* out_rows, int out_cap, int* out_count, int threads,
                     const double* gmc_warp, y7t_stream stream);

/* BoT-SORT (tracker/botsort.py:313-493, tracker kind Y7T_TRACKER_BOTSORT, Kalman kind botsort): `gmc_warp` / `gmc_warps[b]` is the
 * 2x3 camera-motion matrix of the frame (row-major, 6 doubles in DEVICE memory; NULL = no compensation) that the reference's
 * GMC.apply returns (botsort.py:13-248; the 'ecc' method is y7t_ecc_align below, ORB / SIFT / file are out of scope); the step applies multi_gmc
 * (botsort.py:250-269) to the predicted pool and the unconfirmed tracks.  Same op on its own: */
int y7t_kf_multi_gmc_f64(double* mean, double* cov, const double* warp, int N, y7t_stream stream);

/* Camera-motion ESTIMATION: GMC(method='ecc') of the reference (tracker/botsort.py:78-109 = cv2.findTransformECC, MOTION_EUCLIDEAN, identity start) in exact
 * arithmetic (DESIGN.md section 4 "GMC / ECC" states the specification and what is not claimed against OpenCV's fixed-point 8-bit routines).
 * A PLANE is h x w pixels of 16 bytes {I, gx, gy, 0} float32 (the gray level and its central-difference gradients), 16-byte aligned, in DEVICE memory.
 * y7t_ecc_prepare_u8: bgr = (H, W, 3) uint8 frame (device) -> the plane of (H / downscale) x (W / downscale) pixels: gray, 3x3 Gaussian blur sigma 1.5, bilinear
 *   resize, gradients, in one launch.  downscale >= 1; 1 skips blur and resize (botsort.py:86).
 * y7t_ecc_workspace_bytes: bytes of DEVICE workspace (8-byte aligned) one alignment of h x w planes needs; no initialisation required.
 * y7t_ecc_align: warp_out6_f64 (6 doubles, device, row-major 2x3) = the Euclidean warp that maps template coordinates into the image, identity when the
 *   alignment fails (botsort.py:104-107); status_out (4 doubles, device) = {iterations run, Y7T_ECC_* flag, final rho, |rho - rho_last|}.  At most max_iters
 *   iterations, stopping when |rho - rho_last| < eps as OpenCV does; eps < 0 never stops early.  motion other than Y7T_ECC_MOTION_EUCLIDEAN: Y7T_E_ARG.
 *   Asynchronous: max_iters + 3 launches on `stream`, nothing is read back; the same inputs give the same bits on every run.
 * y7t_ecc_iteration_sums_f64 (tests): the 21 combined sums of ONE iteration at the parameters (theta, tx, ty) -> sums_out21_f64 (device): N, sum I, sum I^2,
 *   sum T, sum T^2, sum IT, sum J (3), sum J I (3), sum J T (3), sum J J^T (00 01 02 11 12 22) over the mask. */
enum { Y7T_ECC_MOTION_TRANSLATION = 0, Y7T_ECC_MOTION_EUCLIDEAN = 1, Y7T_ECC_MOTION_AFFINE = 2, Y7T_ECC_MOTION_HOMOGRAPHY = 3 };   /* cv2.MOTION_* */
enum { Y7T_ECC_STATUS_CONVERGED = 1, Y7T_ECC_STATUS_EXHAUSTED = 2, Y7T_ECC_STATUS_FAILED = 3 };
int y7t_ecc_prepare_u8(const uint8_t* bgr, int H, int W, int downscale, void* plane_out, y7t_stream stream);
int y7t_ecc_workspace_bytes(int h, int w, size_t* out);
int y7t_ecc_align(const void* tmpl_plane, const void* img_plane, int h, int w, int motion, int max_iters, double eps, void* workspace,
                  double* warp_out6_f64, double* status_out, y7t_stream stream);
int y7t_ecc_iteration_sums_f64(const void* tmpl_plane, const void* img_plane, int h, int w, double theta, double tx, double ty, void* workspace,
                               double* sums_out21_f64, y7t_stream stream);

/* Camera-motion ESTIMATION from features: GMC.applyFeaures of the reference (tracker/botsort.py:111-235: FAST corners, ORB descriptors, Hamming 2-NN matching, three
 * filters, estimateAffinePartial2D with RANSAC) as a specification of our own in exact arithmetic -- DESIGN.md section 4 "GMC / features" states it and what is not
 * claimed against OpenCV.  A STATE holds the keypoints and descriptors of one frame in DEVICE memory (16-byte aligned, y7t_orb_state_bytes(max_keypoints) bytes):
 * a 32-byte header of ints {n, corners found, truncated, h, w}, max_keypoints descriptors of 32 bytes, max_keypoints keypoints {x, y} (ints, row-major order).
 * y7t_orb_workspace_bytes: bytes of DEVICE workspace (16-byte aligned, no initialisation) that an extraction and an estimate on h x w planes need.
 * y7t_orb_extract_u8: bgr = (H, W, 3) uint8 frame (device); dets = n_dets rows of 6 float32 as y7t_tracker_step takes them (device; tlbr first, full-resolution
 *   pixels; n_dets == 0: no boxes), whose boxes are masked out as botsort.py:129-132 does -> state_out for the plane of (H / downscale) x (W / downscale) pixels,
 *   both sides in 63 .. 8192; at most max_keypoints (1 .. 65536) keypoints, the first in row-major order (the header's `truncated` tells).  Seven launches.
 * y7t_orb_estimate: warp_out6_f64 (6 doubles, device, row-major 2x3 [[a, -b, tx], [b, a, ty]], translation in full-resolution pixels) = the similarity from the
 *   previous frame's coordinates to the current one's, the identity unless the flag is 0; status_out6_f64 (6 doubles, device) = {n_prev, n_cur, good matches,
 *   inliers, Y7T_ORB_* flag, truncated (bit 0 current, bit 1 previous state)}.  h, w, downscale, max_keypoints: as the two states were extracted.  Four launches;
 *   nothing is read back, the counts stay in device memory; the same inputs give the same bits on every run.
 * y7t_orb_tap_layout (tests): the byte offsets in the workspace of {plane, FAST scores, kept corners, smoothed plane (h x w uint8 each), row counts, row offsets
 *   (h ints each), moments (max_keypoints x {m10, m01} ints), best-two matches (x {j1, d1, j2, d2} ints), good matches (x {px, py, cx, cy} ints), the estimate's
 *   header (ints {good, flag, survivors of the first two filters, winning hypothesis, inliers}), inlier counts of the 2000 hypotheses (ints)} and the total. */
enum { Y7T_ORB_STATUS_OK = 0, Y7T_ORB_STATUS_NO_MATCHES = 1, Y7T_ORB_STATUS_NOT_ENOUGH = 2, Y7T_ORB_STATUS_NO_MODEL = 3 };
int y7t_orb_workspace_bytes(int h, int w, int max_keypoints, size_t* out);
int y7t_orb_state_bytes(int max_keypoints, size_t* out);
int y7t_orb_extract_u8(const uint8_t* bgr, int H, int W, int downscale, const float* dets, int n_dets, int max_keypoints, void* workspace, void* state_out,
                       y7t_stream stream);
int y7t_orb_estimate(const void* prev_state, const void* cur_state, int h, int w, int downscale, int max_keypoints, void* workspace, double* warp_out6_f64,
                     double* status_out6_f64, y7t_stream stream);
int y7t_orb_tap_layout(int h, int w, int max_keypoints, size_t* offsets12);

/* C-BIoU (tracker/c_biou_tracker.py:212-353, tracker kind Y7T_TRACKER_C_BIOU; the Kalman kind of y7t_tracker_init is ignored): no motion model, three
 * IoU associations of buffered boxes.  Same pool blob, same layout and the same entry points as SORT / ByteTrack: y7t_tracker_step, y7t_tracker_step_frames,
 * y7t_tracker_step_batch (a batch may mix C-BIoU pools with the others).  A slot's `cov` storage holds the track's last 6 boxes, its two motion states and
 * buffered boxes instead of a covariance.  n < 0 (update_without_detection) on a pool whose confirmed-tracked + lost lists are not empty sets status bit 16
 * (the reference's update_without_detection needs a Kalman mean and fails there) and changes nothing; with an empty pool it advances the frame.  The lost
 * list is never aged (as in the reference): size cap_tracks for the length of the sequence -- an overflow sets status bit 1.
 * y7t_tracker_step_deepsort refuses a C-BIoU pool: Y7T_E_STATE and status bit 8. */

/* UAVMOT (tracker/uavmot.py:109-256, tracker kind Y7T_TRACKER_UAVMOT; Kalman kinds default / botsort / strongsort): ByteTrack with a first association
 * at 0.7 that is re-solved at 0.8 on the fused cost 0.98 * IoU distance + (1 - 0.98) * structure distance (y7t_structure_distance_f64) unless it matched
 * nothing or only the pair (0, 0); the second association's unmatched indices mark strack_pool[idx] lost, as in the reference.  Same pool blob, same
 * layout and the same entry points as ByteTrack: y7t_tracker_step, y7t_tracker_step_frames, y7t_tracker_step_batch (a batch may mix UAVMOT pools with
 * the others).  The structure vectors of a frame (3 doubles per pool track and per detection) live in the blob's dense-LAP work array, which holds
 * (cap_t + max(cap_t, cap_d)) x 40 bytes.  y7t_tracker_step_deepsort refuses a UAVMOT pool: Y7T_E_STATE and status bit 8. */

/* DeepSORT (tracker/deepsort.py:79-227, tracker kind Y7T_TRACKER_DEEPSORT): appearance + motion.  Next to the pool blob the tracker owns
 * a FEATURE STATE (y7t_deepsort_feature_bytes, y7t_deepsort_init): per slot the last `budget` appearance vectors of the track
 * (STrack.features, basetrack.py:97-103,324-332; budget = store_features_budget = 100) plus per-frame scratch.
 * y7t_tracker_step_deepsort = DeepSORT.update for one frame:
 *   det_feats   n x feat_dim float32, row j = what DeepSORT.get_feature (deepsort.py:19-41 -> the ReID network) returns for detection row j
 *               (only rows with conf > conf_thresh are read)
 *   launches: normalise the features, nearest_embedding_distance (tracker/matching.py:105-127) for every live slot (one workgroup per
 *   slot), then ONE workgroup for matching_cascade with gate_cost_matrix (matching.py:216-277, deepsort.py:43-66), the two IoU
 *   associations and the list bookkeeping.  update_without_detection: y7t_tracker_step(state, NULL, -1, ...) as for every tracker. */
size_t y7t_deepsort_feature_bytes(int cap_tracks, int cap_dets, int feat_dim, int budget);
int y7t_deepsort_init(void* feat_state, size_t bytes, int cap_tracks, int cap_dets, int feat_dim, int budget, y7t_stream stream);
int y7t_tracker_step_deepsort(void* state, void* feat_state, int cap_tracks, const float* dets, int n, const float* det_feats, double* out_rows,
                              int out_cap, int* out_count, int threads, y7t_stream stream);

/* StrongSORT (tracker/strongsort.py:91-250, tracker kind Y7T_TRACKER_STRONGSORT; Kalman kinds default / strongsort -- tracker/track.py:70-71 sets
 * strongsort, the NSA filter): the first and the unconfirmed association solve the fused cost gamma * IoU distance + (1 - gamma) * appearance distance
 * at 0.7, the appearance distance being matching.embedding_distance(..., 'euclidean') (tracker/matching.py:84-103: np.maximum(0, scipy cdist) of
 * features[-1] in float64); between them an IoU association at 0.5 whose unmatched indices mark strack_pool[idx] lost, as in the reference.  The
 * pool blob keeps its layout and size.  Next to it the tracker owns a FEATURE STATE of its own (y7t_strongsort_feature_bytes, y7t_strongsort_init):
 * per slot ONE float32 vector of feat_dim (STrack.features with use_avg_of_feature=True, basetrack.py:324-332: the raw vector of the track's first
 * detection, then smooth = 0.9 * smooth + (1 - 0.9) * f / |f|, smooth /= |smooth|, all float32), the frame's float64 appearance matrix
 * (cap_tracks x cap_dets), the frame's list of pending vector stores, and a header whose status word sits at byte 20 as in DeepSORT's
 * (bit 2: the feature state is smaller than the pool it is stepped with; bit 16: more queued vectors than detections).  gamma = opts.gamma.
 * y7t_tracker_step_strongsort = StrongSORT.update for one frame, n known on the host as for DeepSORT:
 *   det_feats   n x feat_dim float32, row j = what StrongSORT.get_feature (strongsort.py:66-89 -> OSNet x0.25 on 256 x 128 crops) returns for
 *               detection row j, NOT normalised (rows with conf <= conf_thresh are never read)
 *   gmc_warp    the frame's 2x3 camera-motion matrix (what GMC(method='ecc').apply returns, out of scope; 6 doubles in DEVICE memory) or NULL for no
 *               compensation; multi_gmc is applied to strack_pool BEFORE the Kalman prediction and not to the unconfirmed tracks (strongsort.py:138-145)
 *   launches (three, on `stream`): the Euclidean distances of every slot of the tracked / lost lists to every detection above the threshold (a grid
 *   over list entries x 64-detection tiles; each pair's sum is the sequential float64 chain of cdist); ONE workgroup for multi_gmc, multi_predict, the
 *   three associations and the list bookkeeping; a wave per queued vector for the moving averages of the updated tracks and the raw copies of the new
 *   ones (re_activate keeps a track's vector).  update_without_detection: y7t_tracker_step(state, NULL, -1, ...) as for every tracker.
 * (For this kind that call runs StrongSORT's own program without a feature state: its tracked and lost lists may share a track, which strack_pool holds once.)
 * Misuse is refused with Y7T_E_STATE and status bit 8 in the pool: y7t_tracker_step with detections and y7t_tracker_step_frames on a StrongSORT pool
 * (y7t_tracker_step_batch: status bit 8 and no rows for that pool of the batch, whatever its n_dets; the launch cannot see its pools' kinds on the host,
 * so it returns 0 as for a DeepSORT pool), y7t_tracker_step_deepsort on a StrongSORT pool, y7t_tracker_step_strongsort on a pool of another kind.  Frames depend on each
 * other through the smoothed vectors, so there is no multi-frame or batch form: a host loop of the three launches is the form. */
size_t y7t_strongsort_feature_bytes(int cap_tracks, int cap_dets, int feat_dim);
int y7t_strongsort_init(void* feat_state, size_t bytes, int cap_tracks, int cap_dets, int feat_dim, double gamma, y7t_stream stream);
int y7t_tracker_step_strongsort(void* state, void* feat_state, const float* dets, int n, const float* det_feats, double* out_rows, int out_cap,
                                int* out_count, int threads, const double* gmc_warp, y7t_stream stream);

/* BoT-SORT with its appearance branch (tracker/botsort.py:313-493 with use_apperance_model = True, tracker kind Y7T_TRACKER_BOTSORT_REID; Kalman kind botsort
 * only; the pool blob has the layout and size of a BoT-SORT pool): the first (0.9) and the unconfirmed (0.7) association solve equations 12-13 of the BoT-SORT
 * paper, cost = min(IoU distance, App) with App = 0.5 * (1 - cosine of the track's smoothed vector and the detection's vector), App = 1 where the IoU distance
 * exceeds theta_iou and App = 1 where App exceeds theta_emb (matching.embedding_distance(..., 'cosine'), tracker/matching.py:84-103,165-178: float64 casts of the
 * float32 vectors, each divided by its np.linalg.norm, then the dot product -- here ONE sequential FMA chain per pair); between them the IoU association at 0.5 of
 * every unmatched pool track with the low detections.  High detections are score >= conf_thresh; only they carry a vector.  The cost differs from the IoU distance
 * only on pairs at or under theta_iou, so a cosine is taken for those pairs alone: the step walks its box pairs, files them in a table and evaluates a lane per pair.
 * Next to the pool the tracker owns a FEATURE STATE (y7t_botsort_reid_feature_bytes, y7t_botsort_reid_init; INTEGRATION.md gives the layout): a 64-byte header that
 * begins like StrongSORT's (status word at byte 20; the frame's count of cosines evaluated at byte 28, theta_iou / theta_emb at bytes 32 / 40, the count of evaluated
 * pairs that theta_emb sent to 1 at byte 48), per slot ONE float32 vector (StrongSORT's store: the raw vector of the track's first detection, then the float32
 * moving average of the normalised vectors; re_activate and a match with a low detection keep it), the pending-store list (two entries per detection), the
 * frame's normalised float64 rows of the listed tracks and of the high detections, and the pair table of the association in flight.  There is no
 * cap_tracks x cap_dets matrix.  Status bits: 2 the feature state is smaller than the pool it is stepped with; 4 a vector with zero or non-finite norm among the
 * frame's rows (the reference hands NaN costs to lapjv there): the frame is NOT stepped, the pool and the vectors stay as they were; 16 more queued vectors than the
 * list holds; 32 more pairs at or under theta_iou than the table holds (8 per track or detection of the capacities, three quarters used).
 * y7t_tracker_step_botsort_reid = BoTSORT.update for one frame, n >= 0 known on the host:
 *   det_feats   n x feat_dim float32, row j = what BoTSORT.get_feature (botsort.py:291-311 -> Extractor: the DeepSORT Net on 128 x 64 crops) returns for detection
 *               row j, NOT normalised (rows with conf < conf_thresh are never read)
 *   gmc_warp    the frame's 2x3 camera-motion matrix (6 doubles in DEVICE memory) or NULL; multi_gmc is applied to strack_pool and to the unconfirmed tracks AFTER
 *               the Kalman prediction (botsort.py:376-382)
 *   launches (three, on `stream`, nothing is read back): a wave per row for the normalised rows; ONE workgroup for multi_predict, multi_gmc, the three
 *   associations with their pair passes and cosines, and the list bookkeeping; a wave per queued vector for the moving averages and the raw copies.
 * update_without_detection: y7t_tracker_step(state, NULL, -1, ...) as for every tracker (the plain program: this pool's lists are disjoint).
 * Misuse is refused with Y7T_E_STATE and status bit 8 in the pool: y7t_tracker_step with detections and y7t_tracker_step_frames on such a pool
 * (y7t_tracker_step_batch: status bit 8 and no rows for that pool of the batch, the call returns 0), y7t_tracker_step_deepsort / y7t_tracker_step_strongsort on such
 * a pool, y7t_tracker_step_botsort_reid on a pool of another kind.  Frames depend on each other through the smoothed vectors: there is no multi-frame or batch form. */
size_t y7t_botsort_reid_feature_bytes(int cap_tracks, int cap_dets, int feat_dim);
int y7t_botsort_reid_init(void* feat_state, size_t bytes, int cap_tracks, int cap_dets, int feat_dim, double theta_iou, double theta_emb, y7t_stream stream);
int y7t_tracker_step_botsort_reid(void* state, void* feat_state, const float* dets, int n, const float* det_feats, double* out_rows, int out_cap,
                                  int* out_count, int threads, const double* gmc_warp, y7t_stream stream);

/* DeepMOT (tracker/deepmot.py:143-324, tracker kind Y7T_TRACKER_DEEPMOT; the pool blob and the Kalman kinds of ByteTrack): ByteTrack whose first association
 * solves 1 - DHN(D) at 0.9, D = matching.ecu_iou_distance(strack_pool, D_high, image shape) cast to float32 and DHN the Deep Hungarian Net (class Munkrs,
 * deepmot.py:10-140): two stacked bidirectional 2-layer GRUs of hidden size 256 over the h x w matrix flattened row-major, then column-major, three linear layers
 * and a sigmoid.  The port is the eval() network: the reference never calls .eval(), so its dropout between the GRU layers is live and its output random.
 *
 * The DHN OBJECT is caller-owned device memory of y7t_dhn_weight_bytes() + y7t_dhn_workspace_bytes(max_h, max_w) bytes at a 256-byte aligned address; several
 * trackers may share one (their frames then run one after the other on one stream).  Supported sizes: any h, w >= 1 with h * w <= max_h * max_w <= 1048576; the
 * workspace holds two T x 512 float32 layer outputs (T = max_h * max_w) and the input projections of one chunk of 2048 positions, so it grows by 4 KiB a position.
 * y7t_dhn_init: `weights` = the y7t_dhn_num_weights() = 4093825 float32 values of the 38 tensors of Munkrs.state_dict() in its order, packed, in host or device
 *   memory (INTEGRATION.md lists the offsets).  Synchronous.  y7t_dhn_release: the object's memory is about to be freed.
 * y7t_dhn_forward_f32: out (h x w, device) = the network's sigmoid output for D (h x w float32, device).  fp32 throughout.  Synchronous: it returns Y7T_E_STATE if
 *   a workgroup of the recurrence waited for a peer past its bound (the recurrence's workgroups exchange the hidden state every step; every wait is bounded).
 * y7t_tracker_step_deepmot = DeepMOT.update for one frame (n >= 0 known on the host; img_h, img_w = ori_img.shape[:2]).  Synchronous.  Y7T_E_STATE with no rows if the
 *   network gave up (pool status bit 64); pool status bit 32 if the frame's pool x high-detection matrix exceeds the object's max_h * max_w.
 * y7t_tracker_step(state, NULL, -1, ...) is update_without_detection.  Misuse is refused with Y7T_E_STATE and status bit 8 in the pool: y7t_tracker_step with
 * detections and y7t_tracker_step_frames on a DeepMOT pool, y7t_tracker_step_batch for such a pool (device-side: the call returns 0), y7t_tracker_step_deepsort /
 * y7t_tracker_step_strongsort on a DeepMOT pool, y7t_tracker_step_deepmot on a pool of another kind. */
size_t y7t_dhn_num_weights(void);
size_t y7t_dhn_weight_bytes(void);
size_t y7t_dhn_workspace_bytes(int max_h, int max_w);
int y7t_dhn_init(void* dhn, size_t bytes, const float* weights, int max_h, int max_w, y7t_stream stream);
int y7t_dhn_release(void* dhn);
int y7t_dhn_forward_f32(void* dhn, const float* D, int h, int w, float* out, y7t_stream stream);
int y7t_tracker_step_deepmot(void* state, void* dhn, const float* dets, int n, int img_h, int img_w, double* out_rows, int out_cap, int* out_count, int threads,
                             y7t_stream stream);

/* AFLink (tracker/reid_models/AFLink.py: class PostLinker, the appearance-free link model of StrongSORT++; the reference ships the network and never calls it):
 * after a sequence, tracklets that a missed detection or an occlusion split into two ids are joined again from their (frame, x, y) rows alone.
 *
 * The AFLINK OBJECT is caller-owned device memory of y7t_aflink_weight_bytes() + y7t_aflink_workspace_bytes(max_tracklets, max_rows, max_pairs) bytes at a
 * 256-byte aligned address.  Capacities: 1 <= max_tracklets <= 32768, max_rows >= 1 (the table stays the caller's: nothing is kept per row today), 1 <= max_pairs
 * <= 2^24.  The workspace holds the activations of one chunk of min(max_pairs, 2048) pairs (72 KiB a pair: 144 MiB at most) and two integers a tracklet.
 * y7t_aflink_init: `weights` = the y7t_aflink_num_weights() = 1075266 float32 values of the float tensors of PostLinker().state_dict() in its order (the
 *   num_batches_tracked entries left out), packed, in host or device memory (INTEGRATION.md lists the offsets).  Synchronous.  y7t_aflink_release: the object's
 *   memory is about to be freed.
 * y7t_aflink_score_pairs_f32: scores[p] = softmax(PostLinker(x1[p], x2[p]))[1] in eval mode for x1, x2 (P x 30 x 3 float32, device; columns frame, x, y as the pair
 *   transform leaves them), any P >= 0.  fp32 throughout; no atomics, bit-identical from call to call.  Asynchronous.
 * y7t_aflink_candidates: the whole device side of AFLink.link.  rows: [frame, x, y] float64 rows of n_tracklets tracklets, each a run sorted by frame; row_offsets:
 *   n_tracklets + 1 int32 (device).  Every ordered pair (i, j), i != j, with thrT0 <= first_frame(j) - last_frame(i) < thrT1 and not thrS < the distance of i's
 *   last and j's first position (float64) is a candidate; candidates are compacted in row-major (i, j) order into pairs_out (max_pairs x 2 int32), transformed
 *   (former: last 30 rows, zero rows in front; latter: first 30, zero rows behind; per column min / max over the 60 rows, (x - (max + min) / 2) / ((max - min) / 2
 *   + 1e-5) in float64, cast to float32) and scored into scores_out (max_pairs float32).  x1_out / x2_out (max_pairs x 90 float32) receive the transformed blocks, or
 *   NULL.  count_out (int32): the number of candidates; status_out (int32): bit 0 = more candidates than max_pairs -- the first max_pairs are listed and scored and
 *   the caller must not use them as the whole list.  Everything stays on the device: asynchronous, no read-back.
 * Errors: Y7T_E_ARG (a null pointer, a misaligned or too small object, a capacity out of range), Y7T_E_STATE (an address y7t_aflink_init never saw),
 * Y7T_E_CAPACITY (n_tracklets > max_tracklets). */
size_t y7t_aflink_num_weights(void);
size_t y7t_aflink_weight_bytes(void);
size_t y7t_aflink_workspace_bytes(int max_tracklets, int max_rows, int max_pairs);
int y7t_aflink_init(void* obj, size_t bytes, const float* weights, int max_tracklets, int max_rows, int max_pairs, y7t_stream stream);
int y7t_aflink_release(void* obj);
int y7t_aflink_score_pairs_f32(void* obj, const float* x1, const float* x2, int P, float* scores, y7t_stream stream);
int y7t_aflink_candidates(void* obj, const double* rows, const int* row_offsets, int n_tracklets, double thrT0, double thrT1, double thrS, int* pairs_out,
                          float* x1_out, float* x2_out, float* scores_out, int* count_out, int* status_out, y7t_stream stream);

/* GSI, the Gaussian-smoothed interpolation of StrongSORT++ (the reference ships no GSI code: `use_GSI` is never read in tracker/strongsort.py; the procedure is
 * this project's restatement of the StrongSORT release's GSI.py, DESIGN.md section 4 "GSI"): after a sequence, the short gaps a missed detection leaves in a
 * track are filled linearly and every track is smoothed by a Gaussian-process regression over its frames.  float64 throughout; no atomics; results are
 * bit-identical from call to call and a track's result does not depend on the other tracks.
 *
 * A table of tracks is `runs`: float64 rows [frame, x, y, w, h], the tracks' rows one run after the other, every run sorted by frame with no frame twice, and
 * `offsets`: n_tracks + 1 int32, run k = rows [offsets[k], offsets[k + 1]).  Both in device memory.
 *
 * The GSI OBJECT is caller-owned device memory of y7t_gsi_workspace_bytes(max_tracks, max_rows, max_len) bytes at a 256-byte aligned address.  Capacities:
 * 1 <= max_tracks <= 32768 = the tracks one group of launches takes (a longer table is taken in groups of max_tracks, with the same result), max_rows >= 1 = the
 * rows of a table after interpolation, 1 <= max_len <= 4096 = the rows of its longest track after interpolation.  The workspace holds one integer a track and a
 * pool of matrix slots for the tracks longer than 128 rows (at most 512 MiB); y7t_gsi_workspace_bytes returns 0 for capacities out of range.
 * y7t_gsi_init / y7t_gsi_release: as for the AFLink object (release: the object's memory is about to be freed).
 * y7t_gsi_interpolate: for consecutive rows of a track at frames f0 < f1 with f0 + 1 < f1 < f0 + interval every frame f in between receives a row, its x, y, w, h
 *   = v0 + (v1 - v0) / (f1 - f0) * (f - f0) evaluated in exactly that order (no fused multiply-add).  runs_out (max_rows x 5 float64): the runs with their gaps
 *   filled; offsets_out (n_tracks + 1 int32): their offsets; src_out (max_rows int32): for every output row the input row it is (a new row: the row at f0);
 *   count_out (int32): the number of output rows; status_out (int32): bit 0 = more than max_rows output rows (the first max_rows are written), bit 1 = a track is
 *   longer than max_len afterwards.  Everything stays on the device: asynchronous, no read-back.
 * y7t_gsi_smooth: for every track of n rows at frames t, with its length scale len_scale[k] (float64, device; the release's is
 *   clip(tau * log(tau^3 / n), 1 / tau, tau^2), computed by the caller): K[i][j] = exp(-0.5 * ((t_i - t_j) / len_scale)^2), A = K + reg I (reg = 1e-10 is
 *   GaussianProcessRegressor's default), A = L L^T, a = A^-1 Y for Y = the columns x, y, w, h; out (rows x 4 float64) = K a.  `longest` = the rows of the longest
 *   track as the caller knows them: above max_len the call is refused before any launch (Y7T_E_CAPACITY).  status_out: one int32 per track, 0 = smoothed;
 *   bit 0 = a non-positive pivot, bit 1 = the track is longer than `longest`, bit 2 = no launch reached it (more rows than max_rows); with any bit set the
 *   track's columns are copied to `out` as they came -- no NaN travels on.  Asynchronous, no read-back.
 * Errors: Y7T_E_ARG (a null pointer, a misaligned or too small object, a capacity out of range, reg < 0), Y7T_E_STATE (an address y7t_gsi_init never saw),
 * Y7T_E_CAPACITY (longest > max_len). */
size_t y7t_gsi_workspace_bytes(int max_tracks, int max_rows, int max_len);
int y7t_gsi_init(void* obj, size_t bytes, int max_tracks, int max_rows, int max_len, y7t_stream stream);
int y7t_gsi_release(void* obj);
int y7t_gsi_interpolate(void* obj, const double* runs, const int* offsets, int n_tracks, int interval, double* runs_out, int* offsets_out, int* src_out,
                        int* count_out, int* status_out, y7t_stream stream);
int y7t_gsi_smooth(void* obj, const double* runs, const int* offsets, const double* len_scale, int n_tracks, int longest, double reg, double* out,
                   int* status_out, y7t_stream stream);

/* Annotated frames, tracker/track.py:176-177, 275-340 (plot_img, save_videos; --save_images / --save_videos): the overlay and a baseline JPEG encoder for what
 * it returns, both on the device (DESIGN.md section 4 "Rendering" is the specification; csrc/y7t_render.h states the arithmetic).  Integer arithmetic decides
 * every pixel and every bit, no global atomics: results are bit-identical from call to call and a frame's do not depend on the rest of the batch.
 *
 * y7t_render_draw: frames (B, H, W, 3) uint8 BGR -> out, the same shape (another buffer; the frames are not modified).  `tracks`: the rows of all frames, frame b's
 *   rows [offsets[b], offsets[b + 1]) (offsets: B + 1 int32); a row is y7t_render_track: the box as tlwh, the id (the colour: get_color of track.py:311-316) and
 *   the label the host assembled.  A track draws the 3-pixel outline of the rectangle int(x), int(y), int(x + w), int(y + h) in its colour, then its label in
 *   (255, 164, 0) with this project's 8 x 12 bitmap font (csrc/y7t_font.h), the baseline at the rectangle's first corner; the tracks draw in row order and a pixel
 *   keeps the last primitive that covers it.  Not cv2's rasteriser and not its Hershey glyphs.  frames, out and tracks are 4-byte aligned; H, W, B <= 65535.
 * The JPEG ENCODER is caller-owned device memory of y7t_jpeg_bytes(H, W, subsampling, max_batch, &out_bytes) bytes at a 256-byte aligned address (0: sizes out of
 *   range or a batch whose image could pass 2 GiB); out_bytes = the bytes the `out` buffer of a batch of max_batch frames must have: every MCU row has a slot for
 *   its longest possible code, so nothing can overflow.  y7t_jpeg_init writes the tables and the file header for (quality 1 .. 100, subsampling); y7t_jpeg_release:
 *   the object's memory is about to be freed.
 * y7t_jpeg_encode: frames (B, H, W, 3) uint8 BGR, B <= max_batch -> out: the B files one after the other, file b = bytes [lens[b], lens[b + 1]) (lens: B + 1 int32,
 *   device).  Sequential baseline DCT, 8 bit, YCbCr, JFIF APP0, the Annex K Huffman tables, the Annex K quantisation tables scaled the IJG way, a restart interval of
 *   one MCU row (DRI, RST0 .. 7 between the rows), frames padded to whole MCUs by edge replication.  Three launches, no read-back, asynchronous.
 * Errors: Y7T_E_ARG (a null or misaligned pointer, sizes out of range, a buffer too small), Y7T_E_STATE (an address y7t_jpeg_init never saw), Y7T_E_CAPACITY
 * (B > max_batch). */
enum { Y7T_JPEG_SUB_420 = 0, Y7T_JPEG_SUB_444 = 1 };
#define Y7T_RENDER_LABEL_BYTES 24
typedef struct y7t_render_track {
    float x, y, w, h;                                   /* tlwh */
    int32_t id;
    int32_t len;                                        /* bytes of the label, 0 .. 24 */
    unsigned char label[Y7T_RENDER_LABEL_BYTES];        /* CATEGORY_DICT[cls] + '-' + str(id), printable ASCII */
} y7t_render_track;                                     /* sizeof == 48 */
int y7t_render_draw(const uint8_t* frames, int B, int H, int W, const void* tracks, const int* offsets, uint8_t* out, y7t_stream stream);
size_t y7t_jpeg_bytes(int H, int W, int subsampling, int max_batch, size_t* out_bytes_host);
int y7t_jpeg_init(void* obj, size_t bytes, int H, int W, int quality, int subsampling, int max_batch, y7t_stream stream);
int y7t_jpeg_release(void* obj);
int y7t_jpeg_encode(void* obj, const uint8_t* frames, int B, uint8_t* out, size_t out_bytes, int* lens, y7t_stream stream);

/* Frames from JPEG files, tracker/tracker_dataloader.py:94-104 (the loader's cv2.imread): a baseline JPEG DECODER on the device, the encoder's mirror (DESIGN.md
 * section 4 "JPEG decoding" is the specification; csrc/y7t_jpegdec.h states the arithmetic).  The frame is, byte for byte, what libjpeg-turbo returns with its
 * defaults (the accurate integer inverse DCT, "fancy" chroma upsampling, YCbCr -> RGB), stored as B, G, R.  A call takes B files of ONE geometry (H, W,
 * components, sampling); integer arithmetic decides every bit, no atomics, no read-back, bit-identical from call to call, a file's frame independent of the batch.
 * The DECODER is caller-owned device memory of y7t_jpegdec_bytes(...) bytes at a 256-byte aligned address (0: arguments out of range): H, W <=
 *   Y7T_JPEGDEC_MAX_SIDE; components 3 with Y7T_JPEGDEC_444 / _422 / _420 (luminance 1x1, 2x1, 2x2 over chrominance 1x1) or 1 with Y7T_JPEGDEC_GRAY; max_file_bytes
 *   <= 2^28: the longest file a call may hold; subseq_bytes: the stuffed bytes of the scan a lane decodes, a multiple of 4 in Y7T_JPEGDEC_SUBSEQ_MIN .. 4096, 0 =
 *   Y7T_JPEGDEC_SUBSEQ_DEFAULT.  y7t_jpegdec_release: the object's memory is about to be freed.
 * y7t_jpegdec_decode: files (device): the B files' bytes, file b at descs[b].file_off; descs (HOST, copied before the call returns): what a parser of the markers
 *   found, see y7t_jpegdec_desc (tracker/jpeg_decode.py: parse); frames (device, 4-byte aligned) <- (B, H, W, 3) uint8 BGR; status (device, B int32) <- 0, or
 *   Y7T_JPEGDEC_E_* bits for a file whose scan is malformed: its frame then holds the blocks that were decoded before and after the damage, mid-grey where none
 *   was, and no other file of the batch is affected.  Every read of a file is clamped to its bytes and every index to its array: no input can make a kernel read
 *   or write elsewhere.  After a call the int32 at byte 256 + 4 * b of the object is the last launch of the synchronisation that found work for file b, plus one.
 *   Launches: the runs of the batch's longest scan (of 256 * subseq_bytes bytes each: those that find their run settled return at once) + 4; asynchronous.
 * Errors: Y7T_E_ARG (a null or misaligned pointer, sizes out of range, a record that points outside its file), Y7T_E_STATE (an address y7t_jpegdec_init never
 * saw), Y7T_E_CAPACITY (B > max_batch, a file longer than max_file_bytes); none of them launches anything. */
enum { Y7T_JPEGDEC_444 = 0, Y7T_JPEGDEC_422 = 1, Y7T_JPEGDEC_420 = 2, Y7T_JPEGDEC_GRAY = 3 };
enum { Y7T_JPEGDEC_E_CODE = 1, Y7T_JPEGDEC_E_TRUNC = 2, Y7T_JPEGDEC_E_COUNT = 4, Y7T_JPEGDEC_E_RANGE = 8, Y7T_JPEGDEC_E_RESTART = 16 };
#define Y7T_JPEGDEC_MAX_SIDE 16384
#define Y7T_JPEGDEC_SUBSEQ_MIN 16
#define Y7T_JPEGDEC_SUBSEQ_DEFAULT 64
typedef struct y7t_jpegdec_desc {
    uint32_t file_off, file_len;          /* the file inside `files`; every other offset counts from the file's first byte */
    uint32_t scan_off, scan_len;          /* the entropy-coded bytes: from behind the SOS header up to the marker that ends the scan */
    uint32_t restart_interval;            /* DRI, in MCUs; 0: none */
    uint32_t dqt_off[4];                  /* by table id: the 64 bytes of an 8-bit quantisation table (zig-zag order); 0: not defined */
    uint32_t dc_off[4], ac_off[4];        /* by table id: a Huffman table's 16 BITS bytes, HUFFVAL behind them; 0: not defined */
    uint8_t tq[4], td[4], ta[4];          /* by component (scan order): the ids of its quantisation, DC and AC table */
} y7t_jpegdec_desc;                                     /* sizeof == 80 */
size_t y7t_jpegdec_bytes(int H, int W, int components, int sampling, int max_batch, size_t max_file_bytes, int subseq_bytes);
int y7t_jpegdec_init(void* obj, size_t bytes, int H, int W, int components, int sampling, int max_batch, size_t max_file_bytes, int subseq_bytes,
                     y7t_stream stream);
int y7t_jpegdec_release(void* obj);
int y7t_jpegdec_decode(void* obj, const uint8_t* files, const y7t_jpegdec_desc* descs, int B, uint8_t* frames, int* status, y7t_stream stream);

/* mAP evaluation of the detector, as the reference's test.py grades a checkpoint: the per-image statistics of test.py:126-209 and ap_per_class / compute_ap of
 * utils/metrics.py:18-106 (DESIGN.md section 4 "mAP evaluation").  No prediction row reaches the host; no atomics; the stored rows do not depend on how the images
 * were split into calls, and two computes over one state give the same bits.
 *
 * The STATE is caller-owned device memory of y7t_map_bytes(cap_rows, nc) bytes at a 256-byte aligned address (0 for cap_rows < 1 or nc outside [1, 65535]): a
 * 256-byte header of int32 words (0: rows stored, 1: images seen, 2: status), nt (int64[nc], targets per class), and per stored row conf (float32), cls (int32) and
 * correct (int32, bit k = IoU > iouv[k]), followed by the workspace of the compute (about 48 bytes a row in all).  y7t_map_layout: out4 = the byte offsets of nt,
 * conf, cls, correct.  y7t_map_init zeroes the counts (it is also the reset); y7t_map_release: the memory is about to be freed.
 * y7t_map_update: one batch.  dets (batch x max_det x 6 float32, of which conf and cls are read), ndets (batch int32), keep (batch x max_det int32) as
 *   y7t_det_postprocess wrote them; cand_boxes: the candidate boxes `keep` indexes (image b's at cand_boxes + b * cand_stride * 4, cand_rows of them valid: xyxy in
 *   network pixels, NOT rounded); targets (L x 6 float32 [image, class, x, y, w, h], normalised, grouped by image) with target_offsets (batch + 1 int32: image b's
 *   rows are [offsets[b], offsets[b + 1])); the batch's img_h, img_w; lb (batch x 5 float32: gain, padx, pady, h0, w0, the layout of y7t_det_postprocess); iouv (10
 *   float32, torch.linspace(0.5, 0.95, 10)).  float32, one rounded operation at a time in torch's order: targets *= (W, H, W, H), xywh2xyxy, scale_coords with the
 *   ratio and pad of lb for targets and predictions, box_iou = inter / ((area1 + area2) - inter).  Every prediction takes its same-class target of largest IoU
 *   (lowest index on a tie) and claims it when that IoU is > iouv[0]; a target's first claimant in row order gets correct = iou > iouv, later ones stay all-false.
 *   Rows are appended in image order.  A call that would pass cap_rows stores nothing -- no rows, no targets, no images -- and sets status bit 0.  max_det <= 1024.
 *   Asynchronous, no read-back.
 * y7t_map_compute: a stable least-significant-digit radix sort of the rows by (class ascending, conf descending, arrival order), then per class and threshold the
 *   integer counts, float64 recall = tpc / (n_l + 1e-16) and precision = tpc / (tpc + fpc), the suffix-maximum envelope with compute_ap's sentinels, np.interp at
 *   np.linspace(0, 1, 101) and the trapezoid sum; for threshold 0 the precision and recall curves over -conf at np.linspace(0, 1, 1000).  Device outputs: ap_out
 *   (nc x 10 float64), p_out and r_out (nc x 1000 float64; a class without targets or without predictions is all zero), nt_out (nc int64), classes_out (nc int32:
 *   the classes that have targets, ascending, then -1), info_out (4 int32: rows, images seen, status, number of such classes).  Asynchronous.
 * Errors: Y7T_E_ARG (a null pointer, a misaligned or too small state, a capacity out of range), Y7T_E_STATE (an address y7t_map_init never saw). */
size_t y7t_map_bytes(int cap_rows, int nc);
int y7t_map_layout(int cap_rows, int nc, size_t* out4);
int y7t_map_init(void* obj, size_t bytes, int cap_rows, int nc, y7t_stream stream);
int y7t_map_release(void* obj);
int y7t_map_update(void* obj, const float* dets, const int* ndets, const int* keep, const float* cand_boxes, int cand_rows, int cand_stride, int batch, int max_det,
                   const float* targets, const int* target_offsets, int img_h, int img_w, const float* lb, const float* iouv, y7t_stream stream);
int y7t_map_compute(void* obj, double* ap_out, double* p_out, double* r_out, long long* nt_out, int* classes_out, int* info_out, y7t_stream stream);

/* byte offsets of the arrays inside a state blob, for host-side views (tracked_stracks, lost_stracks, ...).
 * names/offsets: see y7t_tracker_field_name(i); returns the number of fields. */
int y7t_tracker_layout(int cap_tracks, int cap_dets, int64_t* offsets, int max_fields);
const char* y7t_tracker_field_name(int i);


/* ---------------------------------------------------------------- detector (YOLOv7 forward) ---- */
/* How a conv op's weights are packed -- and therefore which kernel reads them.  The values are ABI: y7t_op::korder carries them, and so do recorded plans.
 * Python mirror: detector/layout.py::WeightLayout (with the packer of each); packers in detector/weights.py, kernels in csrc/. */
typedef enum y7t_weight_layout {
    Y7T_WL_TAP_MAJOR = 0,         /* rows [Cout_pad][K_pad], k = (kh*KW + kw)*Cin + ci; weights.pack itself; the generic kernel (y7t_conv.hip), the patch kernel on large maps */
    Y7T_WL_LINE_MAJOR = 1,        /* the same rows with k in (kh, 64-channel chunk, kw) order (3x3, Cin % 64 == 0); weights.pack itself; y7t_conv.hip, y7t_conv_patch.hip */
    Y7T_WL_PATCH = 2,             /* per K-step the swizzled LDS image of a 128-row (Cout_pad % 128) or 64-row panel; panel_pack; y7t_conv_patch.hip */
    Y7T_WL_PANEL_1X1 = 3,         /* 1x1: per 32-deep K-step one contiguous 128- or 64-row panel; panel_pack_linear; the 32-deep kernel of y7t_conv.hip */
    Y7T_WL_PATCH_S2 = 4,          /* stride-2 3x3: per (16-channel chunk, tap) a 256- or 128-row panel; panel_pack_s2; y7t_conv_patch_s2.hip */
    Y7T_WL_WS64 = 5,              /* the 64 -> 64 3x3 filter bank as MFMA A-fragments; pack_ws; y7t_conv_ws.hip */
    Y7T_WL_WS128 = 6,             /* the 128 -> 128 k 3x3 bank as A-fragments per 128-channel tile, stride 1 and 2; pack_ws128; y7t_conv_ws128.hip */
    Y7T_WL_P8 = 7,                /* 1x1, Cout_pad % 256 == 0: per (channel tile, 64-deep K-tile) the swizzled LDS image of a 256 x 64 panel; panel_pack_p8; y7t_conv_p8.hip */
    Y7T_WL_WS_S2 = 8,             /* the 64 -> 128 3x3 / stride 2 bank as A-fragments; pack_ws_s2; y7t_conv_ws_s2.hip */
    Y7T_WL_PATCH_N64 = 9,         /* Y7T_WL_PATCH with 64-row panels although Cout_pad % 128 == 0 (small maps); panel_pack(narrow); y7t_conv_patch.hip */
    Y7T_WL_PANEL_1X1_N64 = 10,    /* Y7T_WL_PANEL_1X1 with 64-row panels although Cout_pad % 128 == 0; panel_pack_linear(narrow); y7t_conv.hip */
    Y7T_WL_WS_S2_TWIN = 11,       /* Y7T_WL_WS_S2 FOLLOWED by the 128 -> 128 bank of the twin 1x1 convolution that consumes the layer and its 128 biases behind the layer's own:
                                     one launch computes both, Cout / out_* describe the 1x1 layer's output, the tensor between them is never written; pack_ws_s2 then
                                     pack_ws_s2_tail (blob-only layout 12, TWIN_TAIL in detector/layout.py: it never appears in an op); y7t_conv_ws_s2.hip */
    Y7T_WL_COUNT = 12
} y7t_weight_layout;
/* The same choice in the `act` argument of y7t_conv2d_nhwc_f16: bits 0-7 the activation, bit 8 layout 1, bit 9 forces the patch kernel on an eligible 3x3 / stride 1
 * layer whatever its size (tests), bit 8 + L layout L for L = 2 .. 11.  Of several layout bits the highest layout wins. */
#define Y7T_ACT_FORCE_PATCH 512
#define Y7T_ACT_LAYOUT_BITS(layout) ((layout) <= 0 ? 0 : (layout) == 1 ? 256 : 256 << (layout))
static inline int Y7T_ACT_LAYOUT(int act) {      /* the inverse (a function: it loops) */
    for (int l = Y7T_WL_COUNT - 1; l >= 2; --l)
        if (act & Y7T_ACT_LAYOUT_BITS(l)) return l;
    return (act >> 8) & 1;
}

/* One op of a lowered detector graph.  The host (Python) lowers the reference's model graph
 * (models/yolo.py:321-351 forward_once over the yaml layer list, models/yolo.py:443-520 parse_model) into a
 * static launch list over a pre-planned NHWC fp16 activation arena: concat is eliminated (producers write
 * channel slices), BN is folded (utils/torch_utils.py:181-201), weights are packed [Cout_pad][K_pad] fp16. */
enum { Y7T_OP_CONV = 0, Y7T_OP_UPSAMPLE2X = 1, Y7T_OP_MAXPOOL = 2, Y7T_OP_ADD = 3 };
typedef struct y7t_op {
    int32_t type;
    int32_t in_buf, in_ld, in_coff;     /* arena buffer id, channels of that buffer, first channel of the slice */
    int32_t H, W, Cin;                  /* input spatial size and slice channels */
    int32_t out_buf, out_ld, out_coff, out_f32;
    int32_t Ho, Wo, Cout, Cout_pad;
    int32_t KH, KW, stride, pad;        /* conv / pool window */
    int32_t K, K_pad;
    int32_t act;                        /* 0 none, 1 SiLU, 2 LeakyReLU(0.1) */
    int32_t korder;                     /* a y7t_weight_layout: how this op's weights are packed, and therefore which kernel runs it */
    int32_t detect_level;               /* -1: ordinary layer.  l >= 0: the 1x1 conv of Detect level l (models/yolo.py:46); in a fused forward
                                           (y7t_det_forward_fused) its epilogue decodes + filters instead of writing the head tensor */
    int64_t w_off;                      /* element offset into the fp16 weight blob */
    int64_t bias_off;                   /* element offset into the fp32 bias blob */
    /* upsample-on-read (1x1 / stride 1 convs; cfg/deploy/yolov7-w6.yaml:75,89,103: nn.Upsample feeds only a Concat whose consumers are
     * 1x1 convs): channels [up_c0, up_c0 + up_C) of the input slice are not stored at this resolution -- pixel (y, x) reads
     * buffer up_buf (H/2 x W/2, up_ld channels, slice starting at up_coff) at (y >> 1, x >> 1).  up_C == 0: off.
     * Y7T_OP_ADD (Shortcut, models/common.py:80-86: out = a + b, half(float(a) + float(b))) reuses the three fields for its SECOND operand: b is the slice
     * [up_coff, up_coff + Cin) of buffer up_buf with up_ld channels, at the same H x W as the first operand (in_*) and the output; up_c0 / up_C stay 0.  Cin, every
     * ld and every coff must be multiples of 8 and the output slice must not overlap an operand's slice in the same buffer (Y7T_E_ARG, nothing written). */
    int32_t up_buf, up_ld, up_coff, up_c0, up_C, pad0;
} y7t_op;                               /* sizeof == 136 */

typedef struct y7t_det y7t_det;

/* Build an executable plan.  ops/buf_offsets are HOST arrays (copied); arena/weights/bias are DEVICE memory owned by
 * the caller.  buf_offsets[i]: byte offset of arena buffer i, laid out for max_batch images. */
int y7t_det_create(const y7t_op* ops_host, int n_ops, const int64_t* buf_offsets_host, int n_bufs, void* arena, size_t arena_bytes,
                   const void* weights_f16, const void* bias_f32, int max_batch, y7t_det** out);
int y7t_det_destroy(y7t_det* det);

/* models/yolo.py:345 `x = m(x)` for every layer: runs the whole launch list for B images whose input layout
 * (y7t_input_layout) is already in arena buffer 0.  Asynchronous on `stream`.
 * One forward of a detector at a time: the arena, the split-K slabs and the tile counters of the persistent kernels belong to the plan.  Launches on one
 * stream are ordered; a forward (or a piece of one, y7t_det_forward_ops / _fused) issued on another stream than the previous one waits for it on the device.
 * While `stream` is being captured into a hipGraph nothing is recorded or waited for: whoever replays the graph orders the replays.
 * What a replay relies on -- tile counters back at zero, slabs rewritten before they are read, the candidate counters zeroed by a kernel node of the graph, the event skipped --
 * and the test that pins each item: DESIGN.md, section 2 "What a replayed launch list relies on".
 * The kernels address a tensor through 32-bit byte offsets: a conv whose input or output tensor of B images is larger than 2 GiB goes out as several launches over
 * runs of consecutive images (w6 @ 1280 x 1280: the 640^2 / 320^2 layers from 41 images on); results do not depend on where the runs are cut. */
int y7t_det_forward(y7t_det* det, int B, y7t_stream stream);
/* the same launch list in pieces: ops [first, last) of the plan (last < 0: to the end), so that a caller can record an event between
 * two parts of Model.forward_once (models/yolo.py:321-351) -- bench.py starts the previous batch's decode+NMS on another stream once
 * the memory-bound high-resolution layers of the next forward are through.  y7t_det_num_ops: length of the list. */
int y7t_det_num_ops(const y7t_det* det);
/* the eight tile-counter words of op `op` of the plan, copied to the host (a blocking copy: not for a hot path, never while a stream is being captured).  They
 * read zero whenever no forward of the plan is in flight: the last workgroup of a persistent kernel to leave resets them, eager or replayed from a hipGraph. */
int y7t_det_tile_counters(const y7t_det* det, int op, int* out_host);
int y7t_det_forward_ops(y7t_det* det, int B, int first, int last, y7t_stream stream);

/* Fused Detect: describe the Detect levels once (strides / anchors in pixels, models/yolo.py:23-62), then y7t_det_forward_fused runs
 * ops [first, last) like y7t_det_forward_ops, except that the Detect 1x1 convs do not write their (B, ny, nx, na*no) fp32 tensors:
 * their epilogue applies sigmoid + decode (yolo.py:49-56) and the candidate filter of non_max_suppression (utils/general.py:629-662:
 * obj > conf_thres, best class, conf > conf_thres) and appends the survivors to the candidate arrays at the start of `workspace`
 * (layout of y7t_det_postprocess; `cap`, `max_nms` as there).  The candidate counters are zeroed when the range contains op 0.
 * Afterwards call y7t_det_postprocess with head == NULL on the same workspace: it skips its own decode pass.  The (B, 102000, 5+nc)
 * tensor of the reference and the four raw head tensors are never written. */
int y7t_det_set_detect(y7t_det* det, int nl, int na, int no, const float* strides_host, const float* anchors_host);
int y7t_det_forward_fused(y7t_det* det, int B, int first, int last, float conf_thres, int cap, int max_nms, void* workspace,
                          size_t workspace_bytes, y7t_stream stream);

/* TrackerLoader.__getitem__ tail (tracker/tracker_dataloader.py:83-88) + ReOrg (models/common.py:48-53):
 * img: (B,3,H,W) float32 RGB in [0,1] (is_u8 = 0) or (B,H,W,3) uint8 BGR (is_u8 = 1: BGR->RGB and /255 fused);
 * out: NHWC fp16 with ldout channels (16 with reorg: 12 + 4 zero; 8 without: 3 + 5 zero). */
int y7t_input_layout(const void* img, int is_u8, int B, int H, int W, int reorg, void* out_f16, int ldout, y7t_stream stream);

/* The whole front of the forward as one kernel, for plans that start with ReOrg + Conv 3x3 -> 64 (YOLOv7-w6, cfg/deploy/yolov7-w6.yaml:16-17;
 * y7t_det_stem_fusable): raw (B, H0, W0, 3) uint8 BGR frames -> TrackerLoader._letterbox (resize INTER_LINEAR to new_w x new_h at (top, left)
 * of the H x W network input, pad 114; new == source: no resampling) -> BGR->RGB, /255 -> ReOrg -> stem Conv + bias + activation, i.e. what
 * y7t_letterbox_layout_u8 / y7t_input_layout followed by op 0 compute, without the fp16 layout tensor in between.  Continue with
 * y7t_det_forward_ops / y7t_det_forward_fused from op 1.
 * Refusals, nothing written: Y7T_E_STATE if op 0 is not such a stem; Y7T_E_ARG if the plan's image (2 x op 0's map) is no multiple of 32 in H or W (the kernel
 * walks whole 16 x 16 tiles; y7t_det_stem_fusable answers 0 for such a plan), if top + new_h or left + new_w leaves that image, or if B exceeds max_batch. */
int y7t_det_stem_fusable(const y7t_det* det);
int y7t_det_forward_stem_u8(y7t_det* det, const void* frames_u8, int B, int H0, int W0, int new_h, int new_w, int top, int left, y7t_stream stream);

/* TrackerLoader._letterbox (tracker/tracker_dataloader.py:100-130) fused with the layout above, for raw (B,H0,W0,3) uint8 BGR
 * frames: bilinear resize (cv2.INTER_LINEAR geometry: half-pixel centres; float arithmetic, rounded to uint8) to new_w x new_h,
 * placed at (top, left) of the H x W letterboxed image, pad colour 114.  The host computes new_h/new_w/top/left exactly like
 * the reference (auto=True: pad only to the stride multiple). */
int y7t_letterbox_layout_u8(const void* img, int B, int H0, int W0, int H, int W, int new_h, int new_w, int top, int left, int reorg,
                            void* out_f16, int ldout, y7t_stream stream);

/* Detect.forward decode (models/yolo.py:39-57) + non_max_suppression (utils/general.py:607-695; y7t_det_postprocess: classes=None,
 * agnostic=False, multi_label=False -- the tracking path; y7t_det_postprocess_ex: all three through y7t_nms_opts; labels=() always)
 * + scale_coords/clip/round (general.py:319-340, tracker/track.py:234-244), all on the device.
 * head[l]: NHWC fp32 output of the l-th Detect 1x1 conv, [B][ny][nx][na*no].  anchors: [nl][na][2] pixels (host).
 * letterbox: DEVICE [B][5] = gain, pad_w, pad_h, H0, W0.  dets: [B][max_det][6]; ndets: [B];
 * cand_count (may be NULL): [B] candidates above conf_thres (> cap == overflow, caller must check).
 * cap: candidate capacity per image (the number of anchors can never overflow it); the NMS itself runs on the top
 * min(cap, max_nms) candidates like the reference.  workspace: y7t_det_postprocess_workspace_bytes(B, cap, max_nms).
 * head == NULL: the candidates are already in the workspace (y7t_det_forward_fused); ny/nx/strides/anchors are then unused. */
size_t y7t_det_postprocess_workspace_bytes(int B, int cap, int max_nms);
int y7t_det_postprocess(const float* const* head_host_array_of_dev_ptrs, const int* ny, const int* nx, const float* strides,
                        const float* anchors, int nl, int na, int no, int B, float conf_thres, float iou_thres, int max_det,
                        int max_nms, int cap, const float* letterbox, float* dets, int* ndets, int* keep_idx, int* cand_count,
                        void* workspace, size_t workspace_bytes, y7t_stream stream);

/* The remaining arguments of non_max_suppression (general.py:607-608), by value: nothing is allocated, the call stays capturable.
 *   multi_label    with nc > 1 every class j of a row with obj > conf_thres and sigmoid(cls_j) * obj > conf_thres is its own candidate
 *                  (box, that score, j) (general.py:654-656); nc == 1 runs the best-class path (:624).  The candidates of a row share its cidx;
 *                  cand_count counts (row, class) pairs, and a row's pairs are only written below cap.  Decode pass only: the fused Detect
 *                  epilogues keep the best class alone, so head == NULL with multi_label is Y7T_E_STATE.  rows x nc >= 2^31 (the sort key's
 *                  low word and the candidate counter hold row * nc + class): Y7T_E_ARG.
 *   filter_classes != 0: `classes is not None` (:662-663) -- a candidate stays iff bit (c % 32) of class_mask[c / 32] is set for its class c.
 *                  An all-zero mask is classes=[]; ids outside [0, nc) match nothing.  Applied in the rank sort, before the max_nms cut, on
 *                  either candidate source; the candidate arrays and cand_count are NOT filtered (keep_idx addresses the unfiltered slots),
 *                  so further calls on the same workspace with other options each give their own answer.  nc > 32 * Y7T_NMS_MASK_WORDS
 *                  together with a filter: Y7T_E_ARG.
 *   agnostic       the class offset cls * 4096 of the NMS is 0 (:677): one box per object whatever its class.
 * Order of the walk: score descending, then anchor row ascending, then class ascending.  Refusals write nothing.
 * opts == NULL (or all zero) is y7t_det_postprocess exactly: the same kernels, the same launches. */
enum { Y7T_NMS_MASK_WORDS = 8 };
typedef struct y7t_nms_opts {
    int32_t agnostic;
    int32_t multi_label;
    int32_t filter_classes;
    uint32_t class_mask[Y7T_NMS_MASK_WORDS];
} y7t_nms_opts;
int y7t_det_postprocess_ex(const float* const* head_host_array_of_dev_ptrs, const int* ny, const int* nx, const float* strides,
                           const float* anchors, int nl, int na, int no, int B, float conf_thres, float iou_thres, int max_det,
                           int max_nms, int cap, const float* letterbox, float* dets, int* ndets, int* keep_idx, int* cand_count,
                           void* workspace, size_t workspace_bytes, y7t_stream stream, const y7t_nms_opts* opts);

/* Test-time augmentation: Model.forward(x, augment=True) (models/yolo.py:301-317) is three passes -- scales 1, 0.83, 0.67, the middle one flipped left-right --
 * whose decoded rows, brought back to the first pass's coordinates, are concatenated before ONE non_max_suppression.  A pass is: its input (y7t_input_layout for
 * ratio 1, y7t_tta_scale_layout otherwise), the plain launch list of the plan of its size (y7t_det_forward_ops), y7t_det_decode_append; after the last pass
 * y7t_det_postprocess(_ex) with head == NULL on the same workspace.  Passes of one size share a plan and its arena, so a pass is decoded before the next one runs.
 *
 * y7t_tta_scale_layout: x.flip(flip) (0 none, 2 up-down, 3 left-right: the reference's dims) -> scale_img (utils/torch_utils.py:247-257): F.interpolate to
 * hs x ws (bilinear, align_corners=False), pad right and bottom with 0.447 to Hp x Wp -> the input layout of y7t_input_layout (same img / is_u8 / reorg / ldout; a uint8
 * frame is converted as there first), one launch, no intermediate image.  hs = int(H * ratio), Hp = ceil(H * ratio / gs) * gs, computed by the caller in doubles as the
 * reference writes them.  float32 arithmetic in the order csrc/y7t_tta.h states; hs == H copies.  out: B x Hp x Wp (/ 2 with reorg) x ldout fp16, below 2 GiB. */
int y7t_tta_scale_layout(const void* img, int is_u8, int B, int H, int W, int flip, int hs, int ws, int Hp, int Wp, int reorg, void* out_f16, int ldout,
                         y7t_stream stream);

/* The Detect decode + candidate filter of ONE pass (the decode pass of y7t_det_postprocess: obj > conf_thres, best class, conf > conf_thres), with the pass's transform
 * between decode and xywh2xyxy -- xywh / scale (a float32 division), then x = flip_extent - x (flip 3) or y = flip_extent - y (flip 2); flip_extent is the FIRST pass's
 * width or height -- APPENDED to the candidate arrays at the start of `workspace` (layout of y7t_det_postprocess; cap, max_nms as there) with row index
 * row_base + (row inside the pass); row_base = the rows of the passes before (torch.cat(y, 1) order).  first_pass != 0 zeroes the candidate counters first; another pass
 * leaves them.  Past cap the counter grows and nothing is written.  multi_label != 0 with more than one class: Y7T_E_STATE, that form is not built.  Asynchronous, capturable. */
typedef struct y7t_tta_pass {
    float scale;
    int32_t flip;
    float flip_extent;
    int32_t row_base;
} y7t_tta_pass;
int y7t_det_decode_append(const float* const* head_host_array_of_dev_ptrs, const int* ny, const int* nx, const float* strides, const float* anchors, int nl,
                          int na, int no, int B, float conf_thres, int cap, int max_nms, int multi_label, const y7t_tta_pass* pass, int first_pass,
                          void* workspace, size_t workspace_bytes, y7t_stream stream);

/* ---------------------------------------------------------------- ReID embedding (DeepSORT's appearance branch) ---- */
/* DeepSORT.get_feature -> Extractor (tracker/deepsort.py:19-41, tracker/reid_models/deepsort_reid.py:112-153) with OSNet
 * (tracker/reid_models/OSNet.py:282-438) as the network: crops of the frame -> /255, bilinear resize to in_h x in_w (cv2.INTER_LINEAR
 * geometry on the float image), Normalize(mean, std) in the frame's channel order -> the network in eval mode -> (N, feat_dim) float32.
 * Like the detector, the network is a host-lowered op list (BatchNorm folded, fp32 weights in one blob) over a caller-owned arena. */
enum { Y7T_REID_CONV = 0, Y7T_REID_DWCONV3 = 1, Y7T_REID_MAXPOOL3S2 = 2, Y7T_REID_AVGPOOL2 = 3, Y7T_REID_GATE_ACC = 4, Y7T_REID_ADD_RELU = 5,
       Y7T_REID_GAP = 6, Y7T_REID_FC = 7, Y7T_REID_L2NORM = 8 /* x / |x| per crop: Net.forward with reid=True, reid_models/deepsort_reid.py:104 */,
       /* fp16 NHWC buffers (sized in floats like the others: halves / 2), convolutions on the detector's MFMA kernels -- the op list of the
        * reference's DeepSORT embedding network (reid_models/deepsort_reid.py:14-110), tracker/reid.py::lower_deepsort_net_f16:
        * H_PACK fp32 (H, W, 3) -> fp16 (H, W, 16); H_CONV k in {1, 3}, C % 8 == 0, Co % 64 == 0, weights fp16 [Co][round_up(k*k*C, 64)] with
        * k index (kh * k + kw) * C + ci stored at float offset w_off of the blob, fp32 bias [Co] at b_off, no activation; H_MAXPOOL_RELU
        * relu then 3x3 / 2 / pad 1; H_RELU; H_ADD_RELU relu(in + aux); H_GAP_L2NORM mean over the map then x / |x| -> fp32 (C) */
       Y7T_REID_H_PACK = 9, Y7T_REID_H_CONV = 10, Y7T_REID_H_MAXPOOL_RELU = 11, Y7T_REID_H_RELU = 12, Y7T_REID_H_ADD_RELU = 13, Y7T_REID_H_GAP_L2NORM = 14,
       /* The general OSNet path (csrc/y7t_reid_osnet.hip, tracker/reid.py::lower_osnet_f16; DESIGN.md section 4 "OSNet family"): fp16 NHWC maps whose channel
        * counts are padded to a multiple of 16 (pad channels exactly zero), 1x1 weights as MFMA A fragments (reid.py::_frags) at float offset w_off (a multiple
        * of 4), fp32 bias at b_off.
        * H_OS_STEM     in: fp32 (H, W, 3) crops -> raw 7x7 / 2 / 3 conv + bias, fp16 (Ho, Wo, Co), Co <= 64; fragments [Co / 16][14][64][4]
        * H_OS_PW       1x1 C -> Co over the map; relu bit 0 = ReLU; k = residual mode: 0 none, 1 + aux, 2 a second GEMM over aux (s channels, fragments at w2_off)
        * H_OS_LIGHT    level k (0 .. 3) of an OSBlock's four LightConv3x3 chains, s = 4 - k branches, C = mid channels <= 128, p = rows of a strip (0: as many
        *               as fit the LDS); in: conv1's output (k == 0) or the branch buffer, out: the branch buffer (10 slots of H W C halves per crop),
        *               aux: fp32 per-strip channel sums [4][strips][C] per crop; per branch at w_off: fragments | fp32 taps [9][C] | fp32 bias [C]
        * H_OS_GATESUM  in: the branch buffer, aux: the sums -> sum_b gate_b x2_b, fp16 (H, W, C); R <= 8; fc1 [R][C] / bias at w_off / b_off, fc2 [C][R] / bias at
        *               w2_off / b2_off; p as in H_OS_LIGHT
        * H_OS_INSTNORM InstanceNorm2d(affine, eps 1e-5) per (crop, channel) over fp16 (H, W, C), gamma at w_off, beta at b_off, relu; INSTNORM: the same on fp32
        *               maps, for the exact op list (C % 8 == 0)
        * H_OS_AVGPOOL  AvgPool2d(2) on fp16 maps; H_OS_GAPFC mean over the map -> fp16 (C) in aux, then Linear C -> Co + bias (+ ReLU) -> fp32 (Co) */
       Y7T_REID_H_OS_STEM = 15, Y7T_REID_H_OS_PW = 16, Y7T_REID_H_OS_LIGHT = 17, Y7T_REID_H_OS_GATESUM = 18, Y7T_REID_H_OS_INSTNORM = 19, Y7T_REID_H_OS_AVGPOOL = 20,
       Y7T_REID_H_OS_GAPFC = 21, Y7T_REID_INSTNORM = 22 };
typedef struct y7t_reid_op {
    int32_t type;
    int32_t in_buf, out_buf, aux_buf;   /* arena buffers; aux: second addend (ADD_RELU), pooled + gate scratch (GATE_ACC), -1 otherwise */
    int32_t H, W, C;                    /* input map and channels */
    int32_t Ho, Wo, Co;                 /* output map and channels (CONV, pools, FC) */
    int32_t k, s, p;                    /* CONV window */
    int32_t relu;                       /* CONV / DWCONV3 / FC: ReLU after the bias; GATE_ACC: 1 = first branch (overwrite the accumulator) */
    int32_t R, w_kmajor;                /* GATE_ACC: hidden width of the gate MLP (C / 16); CONV: 1 = weights stored (kh, kw, ci, co) instead of (co, kh, kw, ci) */
    int64_t w_off, b_off;               /* float offsets into the weight blob (b_off < 0: no bias); GATE_ACC: fc1 weight / bias */
    int64_t w2_off, b2_off;             /* GATE_ACC: fc2 weight / bias */
} y7t_reid_op;                          /* sizeof == 96 */
typedef struct y7t_reid y7t_reid;
int y7t_reid_create(const y7t_reid_op* ops_host, int n_ops, const int64_t* buf_offsets_host /* in floats */, int n_bufs, void* arena, size_t arena_bytes,
                    const void* weights_f32, int max_crops, int in_h, int in_w, int feat_dim, y7t_reid** out);
int y7t_reid_destroy(y7t_reid* reid);
/* frame_u8: (H, W, 3) uint8 frame in DEVICE memory, boxes: N x 4 float32 tlbr (device) -- or crops_f32 != NULL: N x in_h x in_w x 3 float32
 * crops that are already resized and normalised (device; frame_u8 / boxes ignored).  feats: N x feat_dim float32 (device). */
int y7t_reid_forward(y7t_reid* reid, const void* frame_u8, int H, int W, const float* boxes, int N, const float* crops_f32, float* feats,
                     y7t_stream stream);
/* Crops taken from several frames in one pass (a batch of frames and all their detections -- the throughput mode of BASELINE config 4):
 * frames_u8 = n_frames x (H, W, 3) uint8 contiguous (device), frame_idx[i] = frame of box i (device int32; clamped to [0, n_frames)). */
int y7t_reid_forward_batch(y7t_reid* reid, const void* frames_u8, int n_frames, int H, int W, const float* boxes, const int* frame_idx, int N,
                           float* feats, y7t_stream stream);
/* The MFMA path of config 4 ("ReID conv as MFMA kernel"): OSNet x0_25 on 128 x 64 crops as ONE kernel, one workgroup per crop, every
 * intermediate in LDS, fp16 storage / fp32 accumulate (tracker/reid_models/OSNet.py:223-279,282-438,567-579 with BatchNorm folded).  `blob`
 * (device memory, y7t_reid_fused_blob_size() bytes) holds the parameters in the kernel's consumption order with the 1x1 weights already in
 * MFMA fragment order (host: tracker/reid.py::pack_fused).  Once set, y7t_reid_forward / _batch on frame crops run the fused kernel; the
 * op list above stays the fp32 path (crops_f32 input, other widths / crop sizes).  blob == NULL switches back. */
size_t y7t_reid_fused_blob_size(void);
int y7t_reid_set_fused(y7t_reid* reid, const void* blob, size_t blob_bytes);

/* single fused Conv+bias+act launch (layer-level parity tests, rocprof attribution); same fields as y7t_op but
 * with raw device pointers.  Small launches split K and sum fp32 slabs from ONE process-wide workspace: call it from one stream at
 * a time (a y7t_det owns its own workspace and has no such limit). */
int y7t_conv2d_nhwc_f16(const void* in, int in_ld, int in_coff, int B, int H, int W, int Cin, const void* w_packed, const float* bias,
                        void* out, int out_ld, int out_coff, int out_f32, int Cout, int Cout_pad, int KH, int KW, int stride, int pad,
                        int act, const void* zeros16, y7t_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* Y7T_H */
