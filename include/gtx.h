/*
 * gtx.h -- C ABI of libgtx.so, the MI355X (gfx950) implementation of the geo-trax
 * per-frame extraction hot path.
 *
 * The reference (rfonod/geo-trax) has no FFI of its own: its hot path is two duck-typed
 * Python objects called from one loop, geotrax/extract.py:134-214 --
 *   model.track(frame, **cfg, persist=True)                      extract.py:153
 *   Stabilizer(**cfg).set_ref_frame / .stabilize /
 *     .transform_cur_boxes / .get_cur_trans_matrix               extract.py:139,177-184
 * plus cv2.perspectiveTransform in geotrax/georeference.py:599-605 and
 * cv2.warpPerspective in geotrax/visualize.py:289.
 * Each entry point below names the reference call it stands in for. The Python classes in
 * geo-trax_amd/geotrax_amd/ (YOLO, Stabilizer) bind these symbols with ctypes and keep the
 * reference's method names, argument meaning and error behaviour.
 *
 * Conventions
 *   - every function returns 0 on success or a negative gtx_status; the text of the last
 *     error on the calling thread is available from gtx_last_error();
 *   - no C++ exception crosses this boundary;
 *   - the library owns all device memory; the caller owns every host pointer it passes and
 *     may reuse it as soon as the call returns (calls are synchronous unless named *_submit);
 *   - a context (and everything created from it) is bound to one GPU and is not thread-safe:
 *     one context = one host thread, exactly like the reference's single-threaded loop;
 *   - plain C types only: pointers, sizes, ints, floats, doubles.
 */
#ifndef GTX_H_
#define GTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: gtx_det_config.fp32_split, gtx_tracker_config.{delta_t, inertia, use_byte, min_hits}, gtx_stab_config.clahe appended;
 *    gtx_tracker_replay, gtx_op_clahe, gtx_warp_frame_dev, gtx_yuv420_to_bgr_dev, gtx_stabilizer_{pattern, last_ms} added.
 *    A binder checks gtx_abi_version() against the header it was written for before passing any struct.
 * 3: gtx_stab_config.{affine, filter_type} appended; gtx_tracker_config.type 3 (deepocsort).
 * 4: gtx_op_linear_assignment and gtx_detector_saturated added; GTX_F32S activations live in HBM as (hi, lo) fp16 pairs
 *    (host arrays handed to gtx_op_* stay plain fp32).
 * 5: gtx_feeder_* (read-ahead frame source) added; a saturating split-f16x3 pass is
 *    re-run by the detector through the exact-fp32 kernels (gtx_detector_saturated reports that it happened).
 * 6: gtx_device_open_null_stream, gtx_write_table_f32 / _f64, gtx_write_csv and gtx_track_anchor_walk added.
 * 7: gtx_streams_overlap, gtx_device_mem_info and gtx_sift_stage_ms added; gtx_tracker_config.type 4 (fasttrack) with its parameters appended to the struct.
 * 8: the appearance branch of BoT-SORT on detector-derived vectors (`with_reid: true, model: auto`): gtx_det_config.obj_feats,
 *    gtx_tracker_config.{with_reid, proximity_thresh, appearance_thresh} appended; gtx_detector_features, gtx_tracker_update_feats added;
 *    gtx_tracker_config.type 5 (tracktrack) with its parameters appended; gtx_detector_sparse_box and gtx_detector_pad_skip added.
 * 9: gtx_det_config.arch appended: 1 = RT-DETR (the reference swaps YOLO for RTDETR on the model's yaml, extract.py:222-225);
 *    gtx_tracker_config.alpha_fixed_emb appended, with_reid also read by types 3 (deepocsort) and 5 (tracktrack);
 *    gtx_op_estimate_affine_partial added (GMC methods orb / sift).
 * 10: gtx_ecc_* added (GMC method ecc); gtx_fgmc_* (GMC method orb, stream-ordered) and gtx_gray_half_dev added: new entry
 *     points only, no struct or existing signature changed, so the number stays. gtx_op_psa_attention added and the embedder takes
 *     YOLO11-cls tensors (C2PSA = model.9): the same, the number stays. gtx_det_config.end2end appended at the struct's end (YOLOv10's
 *     one-to-one head; 0 = every earlier behaviour) and gtx_op_dwconv added: the number stays.
 * 11: gtx_op_rt_{linear, layernorm, mha, topk, gather_refer, deform, post} added: RT-DETR's token-side kernels one launcher at a time.
 * 12: gtx_op_{head_gate, head_boxes, nms, v10_select, v10_rows, obj_feats} and gtx_head_level added: the detector's post-pass kernels
 *     one launcher at a time. A detector with more than 2^20 anchors per image is refused (the NMS sort key's anchor field).
 * 13: gtx_stabilizer_{keep_pass, level, candidates} (read-backs of the last extract pass) and gtx_op_orb_{match, ransac} (the
 *     stabilizer's matcher and RANSAC kernel one launch at a time) added. A stabilizer plan is refused per level (more than 8192
 *     keypoints on one level) instead of by max_features; the candidate lists are sized so that no FAST corner can be dropped.
 *     gtx_jpeg_{record_bound, probe, parse, decode_dev, kernel_ms}, gtx_feeder_open_jpeg and feeder kind 2 (compressed JPEG frames) added: new entry
 *     points only, no struct or existing signature changed, so the number stays. gtx_gmc_counts and gtx_op_gmc_{corners, lk, ransac} (the
 *     sparse-optical-flow GMC's kernels one launcher at a time) added: the same, the number stays.
 * 14: gtx_op_sift_{blur, extrema, refine, orient, describe} added: the SIFT kernels one stage at a time. gtx_sift_detect and
 *     gtx_register_images fail (GTX_ERR_UNSUPPORTED) when a stage finds more candidates or keypoints than its list holds, instead of
 *     going on with whichever of them found room. gtx_sift_stab_* (stabilo's sift / rsift stabilizer as a stream-ordered chain on the
 *     detector's gray image) and gtx_op_sift_select (its selection / finalisation / mask kernels on host arrays) added: new entry points
 *     and a struct of their own only, no existing struct or signature changed, so the number stays. gtx_jpeg_enc_{create, destroy,
 *     submit_dev, collect, last_ms}, gtx_jpeg_emit and gtx_op_jpeg_encode (the JPEG frame sink: BGR in HBM -> record -> baseline JPEG)
 *     added: new entry points and an opaque handle only, so the number stays. gtx_op_invert3x3 (the inverse the frame warp uses, on
 *     the host) added: the same, the number stays. gtx_drawer_{create, destroy, draw_dev, last_ms}, gtx_op_draw (the visualize stage's
 *     drawing: a primitive list painted into a frame in HBM) and gtx_dev_copy added: new entry points and an opaque handle only, so the
 *     number stays. gtx_op_pool_down added and arch 0 also takes YOLOv9 t / s / m / c tensors (yolov9.yaml: ELAN1 / RepNCSPELAN4, AConv / ADown,
 *     SPPELAN = model.9, Detect = model.22; told by their names like the other families): the same, the number stays.
 *     gtx_jpeg_enc_{set_entropy, collect_jpeg, entropy_ms}, gtx_jpeg_{picture_bound, header} and gtx_op_jpeg_huff (the JPEG sink's
 *     entropy coder as HIP kernels, opt-in per encoder) added: new entry points only, so the number stays.
 *     gtx_jpeg_{plan_bound, plan, entropy_ms}, gtx_op_jpeg_entropy and gtx_feeder_{set_jpeg_entropy, jpeg_stats} (the JPEG source's entropy decoder as
 *     HIP kernels, opt-in per feeder) added: new entry points only, so the number stays.
 *     gtx_jpeg_{plan_intervals_bound, plan_intervals, restart_ms, emit_restart}, gtx_op_jpeg_restart and gtx_feeder_{set_jpeg_restart,
 *     jpeg_restart_stats} (JPEG frames with restart intervals decoded one lane per interval, opt-in per feeder; the host emitter
 *     writes such frames) added: new entry points only, so the number stays.
 *     gtx_op_georef_tracks, gtx_georef_tracks_ms and gtx_georef_tracks_cfg (the georeference stage's per-track columns as HIP
 *     kernels, opt-in per run) added: new entry points and a struct of their own only, so the number stays.
 *     gtx_op_stem and gtx_op_conv2d_fused (the stem launch, and the convolution launch with its second source, plain output,
 *     saturation flag and fused post / front stages, on host arrays) added: the same, the number stays.
 *     gtx_op_rt_{stem1, pool2, dwconv, upsample2x, tokens_in, mask_invalid} (RT-DETR's map-side kernels one launcher at a time)
 *     added: the same, the number stays.
 *     gtx_plot_canvas_{create, destroy, size, draw, read, dptr, stats}, gtx_op_plot_draw and gtx_op_plot_reduce (the plot stage's
 *     trajectory maps: an image reduced into a canvas in HBM, strokes and discs blended into it) added: new entry points and an
 *     opaque handle only, so the number stays.
 *     gtx_op_head_boxes_r1 added and arch 0 also takes YOLO26 tensors (yolo26.yaml: SPPF with a residual, attention inside model.22, a
 *     Detect of reg_max = 1 read off its last box convolution's four rows, the one-to-one head under gtx_det_config.end2end): a new
 *     entry point only, so the number stays.
 *     gtx_op_head_sparse_box and gtx_sparse_level (the sparse Detect box launch on host arrays) added: a new entry point and a
 *     struct of its own only, so the number stays.
 *     gtx_op_homography_refit (the host refit that ends every robust homography, on host arrays) added: a new entry point only, so
 *     the number stays.
 *     gtx_op_area_attention added and arch 0 also takes YOLO12 tensors (yolo12.yaml: A2C2f blocks with area attention, Detect =
 *     model.21; the tensors tell the graph, gtx_det_config is unchanged): a new entry point only, so the number stays.
 *     gtx_op_stem6 added and arch 0 also takes YOLOv5u tensors (yolov5.yaml with the anchor-free Detect = model.24: a 6x6 stem, C3
 *     blocks; the tensors tell the graph, gtx_det_config is unchanged): a new entry point only, so the number stays.
 *     gtx_op_conv_config added (host only: the kernel a convolution shape is given) and gtx_conv_fused.{res_cstride, res_coff,
 *     in_place} appended at the struct's end (a residual read as a channel slice, and one buffer behind x, residual and y; 0 =
 *     every earlier behaviour), as gtx_det_config.end2end was: the number stays.
 *     gtx_op_gray_resize_dev, gtx_op_gray_resize, gtx_op_gray_resize_ms and gtx_op_gray_working_size (the ORB stabilizer's working-resolution gray image at
 *     any downsample_ratio in (0, 1]) added, and gtx_stab_config.downsample_ratio takes every value of that range instead of 0.5
 *     and 1.0 alone: new entry points and a wider accepted range only, so the number stays. */
#define GTX_ABI_VERSION 14

typedef enum gtx_status {
  GTX_OK = 0,
  GTX_ERR_INVALID = -1,     /* bad argument */
  GTX_ERR_HIP = -2,         /* HIP runtime error */
  GTX_ERR_UNSUPPORTED = -3, /* shape / option outside what the kernels implement */
  GTX_ERR_STATE = -4,       /* call order (e.g. stabilize before set_ref_frame) */
  GTX_ERR_INTERNAL = -5
} gtx_status;

/* GTX_F32S (gtx_op_conv2d only): fp32 arrays like GTX_F32, the convolution runs as split-f16x3 (hi + lo fp16
 * operands, three fp16 MFMAs per product, fp32 accumulate) -- what a detector with fp32_split = 1 uses. */
typedef enum gtx_dtype { GTX_F16 = 0, GTX_F32 = 1, GTX_F32S = 2 } gtx_dtype;

typedef struct gtx_ctx gtx_ctx;
typedef struct gtx_detector gtx_detector;
typedef struct gtx_stabilizer gtx_stabilizer;
typedef struct gtx_tracker gtx_tracker;

/* ------------------------------------------------------------------ library / context */

int gtx_abi_version(void);
/* Last error message of the calling thread ("" if none). Never NULL. */
const char* gtx_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unavailable). */
int gtx_device_count(void);

/* One context per GPU. Replaces the implicit torch device selection the reference leaves to
 * ultralytics (cfg ultralytics.device, geotrax/cfg/default.yaml:236). */
int gtx_ctx_create(int device, gtx_ctx** out);
/* Same, the context's stream gets the device's highest priority when high_priority != 0: for the
 * short kernels of a latency-critical consumer (the stabilizer) running beside the detector. */
int gtx_ctx_create_prio(int device, int high_priority, gtx_ctx** out);
void gtx_ctx_destroy(gtx_ctx* ctx);
int gtx_ctx_synchronize(gtx_ctx* ctx);
/* Makes the device's null stream exist now (one 4-byte fill on it, waited for). The HIP runtime gives every stream its
 * place on one of GPU_MAX_HW_QUEUES (4) hardware queues when the stream is created -- the first four open a queue each,
 * a later one joins the queue that carries the fewest streams (ties: the highest-numbered queue) -- and the null stream
 * takes its place the first time anything synchronous (hipMemcpy, hipMemset: the library's set-up paths) runs. A caller
 * that lays out several contexts for concurrency (geotrax_amd/engine.py StreamPlan) calls this at a fixed point of its
 * creation order, so that which streams share a queue does not depend on when the first set-up copy happens. Idempotent. */
int gtx_device_open_null_stream(int device);
/* hipMemGetInfo of the device: what registration at the reference's size (a 15 000-px orthophoto: ~55 GB of pyramids) reports as its
 * footprint. */
int gtx_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
/* Do kernels on the two contexts' streams run at the same time? One idle wave spins for spin_us microseconds on a's stream
 * (ms_single: host-timed, best of three) and then on both streams at once (ms_pair). Streams that share a hardware queue run
 * in order: ms_pair ~ 2 x ms_single; streams on queues of their own: ms_pair ~ ms_single. The extract engine's stream plan
 * (geotrax_amd/engine.py) is computed from a measured rule of the HIP runtime, not a documented one; this is its self-check. */
int gtx_streams_overlap(gtx_ctx* a, gtx_ctx* b, float spin_us, float* ms_single, float* ms_pair);
/* Raw device memory for callers that keep inputs resident in HBM (bench.py). */
int gtx_dev_alloc(gtx_ctx* ctx, size_t bytes, void** dptr);
int gtx_dev_free(gtx_ctx* ctx, void* dptr);
int gtx_dev_upload(gtx_ctx* ctx, void* dptr, const void* host, size_t bytes);
int gtx_dev_download(gtx_ctx* ctx, void* host, const void* dptr, size_t bytes);
/* Device-to-device copy of `bytes` bytes (both dptrs from gtx_dev_alloc, not overlapping), enqueued on the context's stream; returns
 * without waiting. Replaces ref_frame.copy() of visualisation mode 2 (visualize.py:277, :292): every frame is drawn on a fresh
 * copy of the kept reference frame. */
int gtx_dev_copy(gtx_ctx* ctx, void* dst_dptr, const void* src_dptr, size_t bytes);

/* One planar YUV 4:2:0 (I420) frame in HBM -> packed BGR u8 in HBM: the colour conversion a video decoder applies
 * before extract.py:146 sees the frame (cv2.VideoCapture.read() returns BGR). BT.601 limited range, the fixed-point
 * constants of cv2.cvtColor(COLOR_YUV2BGR_I420), one chroma sample per 2x2 luma block. yuv_dptr: h*w luma bytes, then
 * the U and V planes of ((h+1)/2)*((w+1)/2) bytes each; bgr_dptr: h*w*3 bytes. Enqueued on the context's stream. */
int gtx_yuv420_to_bgr_dev(gtx_ctx* ctx, const void* yuv_dptr, int h, int w, void* bgr_dptr);

/* Read-ahead frame source: the `cap.read()` at the top of the reference's loop (geotrax/extract.py:146) taken off
 * the thread that drives the detector. Frames of an uncompressed file (.y4m payloads, the data block of a .npy) are
 * read by the feeder's own threads with pread() straight into a ring of pinned host slots, copied to a ring of
 * device batches on the feeder's own stream (I420 frames converted to BGR there, as gtx_yuv420_to_bgr_dev does) and
 * handed out in clip order as device pointers of `batch` contiguous BGR frames.
 *   kind: 0 = frames are BGR u8 [h][w][3]; 1 = I420 planes (h*w + 2*((h+1)/2)*((w+1)/2) bytes); 2 = compressed JPEG frames
 *   (gtx_feeder_open_jpeg below).
 *   ring: device batches (and pinned slots x batch) the feeder owns; it reads ahead until all of them are full.
 * gtx_feeder_open_file: deliver the n_frames frames whose payloads start at offsets[i] (delivery order = array order),
 *   read by n_threads reader threads. gtx_feeder_open_push / _push / _finish: the caller's thread supplies host frames
 *   (any source without a flat file layout); push blocks while the ring is full, finish marks the end of the source.
 * gtx_feeder_next: blocks until the next batch's copies are enqueued; *n = frames in it (batch, fewer for the last one,
 *   0 at the end of the source: *dptr = NULL). A read error surfaces here as a negative status after the batches that
 *   preceded it were delivered. gtx_feeder_wait: the consumer context's stream waits for batch `batch_index` to be
 *   resident (no host thread blocks); consumer NULL: the calling thread waits. gtx_feeder_release: the first n_batches
 *   batches have been consumed (the kernels reading them are complete); their slots are read into again.
 * Thread safety: next / wait / release from one consumer thread, push / finish from one producer thread (push_at: any). */
typedef struct gtx_feeder gtx_feeder;
int gtx_feeder_create(int device, int h, int w, int kind, int batch, int ring, gtx_feeder** out);
/* Same, the transfers and conversions run on copy_ctx's stream instead of a stream of the feeder's own (the context must
 * outlive the feeder and be used for nothing else meanwhile). HIP deals streams to a few hardware queues in creation order and
 * streams that share a queue run in order: a caller that creates its streams in a deliberate order (geotrax_amd.engine does)
 * decides this way whose launches the transfers may delay. */
int gtx_feeder_create_on(gtx_ctx* copy_ctx, int h, int w, int kind, int batch, int ring, gtx_feeder** out);
void gtx_feeder_destroy(gtx_feeder* f);
int gtx_feeder_open_file(gtx_feeder* f, const char* path, const int64_t* offsets, int64_t n_frames, int n_threads);
/* The frames are host arrays (decoded footage held in memory, an ndarray [F][h][w][3]): frames[i] points at frame i's bytes,
 * delivery order = array order; the library's reader threads copy them into the pinned ring. The arrays must stay alive and
 * unchanged until the feeder is destroyed. */
int gtx_feeder_open_memory(gtx_feeder* f, const void* const* frames, int64_t n_frames, int n_threads);
int gtx_feeder_open_push(gtx_feeder* f);
int gtx_feeder_push(gtx_feeder* f, const void* frame, size_t bytes);
/* Push mode with several producer threads: frame number i of the source (each number exactly once, any order, any thread;
 * a push blocks while frame i's batch is more than `ring` batches ahead of the consumer). gtx_feeder_finish after the last
 * push has returned. */
int gtx_feeder_push_at(gtx_feeder* f, int64_t i, const void* frame, size_t bytes);
int gtx_feeder_finish(gtx_feeder* f);
/* Abandons the source: worker threads end, a blocked gtx_feeder_push / gtx_feeder_next returns with an error. Call it
 * (and join the pushing thread) before gtx_feeder_destroy when the run is given up half way. */
int gtx_feeder_stop(gtx_feeder* f);
int gtx_feeder_next(gtx_feeder* f, void** dptr, int* n, int64_t* batch_index);
int gtx_feeder_wait(gtx_feeder* f, int64_t batch_index, gtx_ctx* consumer);
int gtx_feeder_release(gtx_feeder* f, int64_t n_batches);

/* JPEG frame source: cv2.VideoCapture.read() (geotrax/extract.py:146) for Motion-JPEG clips (.mjpeg, MJPG .avi) and folders of
 * .jpg frames. Baseline (SOF0) 8-bit Huffman JPEG, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0 in one interleaved scan, with or
 * without DHT (ITU T.81 Annex K.3 tables) and restart intervals; everything else (progressive, arithmetic, 12-bit, CMYK, Adobe
 * RGB / YCCK, other samplings, multi-scan colour, 16-bit DQT) is GTX_ERR_UNSUPPORTED with the marker and the frame number in the
 * message, damaged data GTX_ERR_INVALID: a frame decodes whole or not at all. The host decodes the entropy-coded data into a
 * packed record (csrc/jpeg_parse.hpp: header, one quantisation table per component, a uint32 offset per 8x8 block, one int16
 * stream of zigzag runs); the GPU dequantises, inverts the DCT, upsamples the chroma and converts to BGR with libjpeg's default
 * integer arithmetic (slow-integer IDCT, fancy upsampling, 16-bit YCbCr tables): the bytes of cv2.imread / Pillow. */
/* Replaces cv2.VideoCapture.read(), extract.py:146 (its worst-case record size for an h x w frame; 0 for a bad size). */
size_t gtx_jpeg_record_bound(int h, int w);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (the entropy-decoding half; host only, no context). Decodes bytes[0, n) into
 * record[0, capacity) (4-byte aligned; NULL with capacity 0 asks for the size). *h, *w, *ncomp (1 or 3), *hs, *vs (luma sampling
 * factors) are set once the frame header is read, *needed when the frame decodes. Returns 0 (record filled, *needed bytes),
 * 1 (capacity < *needed: nothing usable was written) or a negative status. `frame` numbers the frame in messages. Output
 * pointers other than `needed` may be NULL. */
int gtx_jpeg_parse(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs, void* record, size_t capacity,
                   size_t* needed);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (its decision whether it can play a picture): the header half of gtx_jpeg_parse
 * alone. bytes[0, n) need only reach the SOS header; 0 when gtx_jpeg_parse would decode this variant, else its negative status
 * and message. A folder of .jpg frames is routed by it (geotrax_amd.frames.DirReader). */
int gtx_jpeg_probe(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (the pixel half): one record (host memory, `bytes` long, as gtx_jpeg_parse
 * filled it) of an h x w frame -> packed BGR u8 [h][w][3] at bgr_dptr, on the context's stream; the sibling of
 * gtx_yuv420_to_bgr_dev. The record is checked on the host first (sizes, monotone offsets, closing offset): a damaged one is
 * GTX_ERR_INVALID before any launch. Returns when the frame is complete. */
int gtx_jpeg_decode_dev(gtx_ctx* ctx, const void* record, size_t bytes, int h, int w, void* bgr_dptr);
/* Timing of what replaces cv2.VideoCapture.read(), extract.py:146: the two kernels of gtx_jpeg_decode_dev `reps` times on the
 * context's stream with events around each (after one untimed pass), and, when yuv_dptr is not NULL (an I420 frame of the same
 * h x w in HBM), gtx_yuv420_to_bgr_dev in the same loop: ms[0] = inverse DCT launch, ms[1] = upsampling + colour launch,
 * ms[2] = the I420 conversion (0 without yuv_dptr), mean milliseconds per launch. tools/jpeg_time.py. */
int gtx_jpeg_kernel_ms(gtx_ctx* ctx, const void* record, size_t bytes, int h, int w, void* bgr_dptr, const void* yuv_dptr, int reps, float ms[3]);
/* Replaces cv2.VideoCapture.read(), extract.py:146, for a feeder of kind 2 (compressed JPEG frames): frame i is lengths[i] bytes
 * at offsets[i] of paths[file_index[i]] (one .mjpeg / .avi file, or one file per frame). n_threads reader threads pread() the
 * compressed bytes and entropy-decode them into the pinned slot (sized for the worst-case record); the copy stream uploads the
 * record's real length and launches the two kernels into the batch slot. A frame that cannot be decoded, or whose size is not
 * the feeder's h x w, surfaces at gtx_feeder_next after the batches before it. With kind 2, gtx_feeder_push / _push_at take one
 * compressed frame of any length. */
int gtx_feeder_open_jpeg(gtx_feeder* f, const char* const* paths, int n_paths, const int32_t* file_index, const int64_t* offsets,
                         const int64_t* lengths, int64_t n_frames, int n_threads);

/* JPEG frame source, the GPU entropy route (opt-in): the Huffman decode of gtx_jpeg_parse moved from the reader threads to HIP
 * kernels (csrc/jpeg_entropy.hip). The host keeps the header walk and the removal of the byte stuffing (the "plan",
 * csrc/jpeg_parse.hpp: header, quantisers, the scan's Huffman tables, the clean entropy-coded segment); the GPU cuts the clean
 * stream into subsequences of `sub_bits` bits, finds every subsequence's entry state by the self-synchronising decode and writes
 * the packed record, byte for byte what gtx_jpeg_parse writes for the same picture. A frame the kernels cannot vouch for (damaged
 * data, or entry states still changing after the enqueued rounds) gets a non-zero status and is decoded by gtx_jpeg_parse, so
 * which frames decode and what an error says do not depend on the route. Frames with a restart interval stay on the host. */
/* Replaces cv2.VideoCapture.read(), extract.py:146 (buffer sizing): the largest plan a decodable frame of h x w can need; 0
 * for a size outside 1..16384. */
size_t gtx_jpeg_plan_bound(int h, int w);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (the header walk; host only, no context): bytes[0, n) -> the plan in
 * out[0, capacity) (4-byte aligned; NULL with capacity 0 asks for the size). *needed receives the plan's size. Returns 0 (plan
 * written), 1 (capacity < *needed, nothing written), 2 (a frame for the host route: a restart interval; *needed is 0) or the
 * negative status and message gtx_jpeg_parse gives for the same header. h, w, ncomp, hs, vs as gtx_jpeg_parse. */
int gtx_jpeg_plan(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs, void* out, size_t capacity,
                  size_t* needed);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (the entropy decode; operator hook for tests and tools): uploads plan[0, bytes)
 * (host memory, as gtx_jpeg_plan wrote it), runs the entropy chain and copies the record at its real length into
 * record[0, capacity). sub_bits: 256, 512, 1024 or 2048, 0 = the production choice; rounds: synchronisation rounds across
 * workgroups to enqueue, 1..64, 0 = the production choice. *status: 0, or bit 0 = invalid data, bit 1 = not converged (no record is
 * returned then and *record_bytes is 0); *rounds_used: rounds in which a workgroup's entry state still changed, round 0 included.
 * Returns 0, 1 (capacity < *record_bytes, nothing copied) or a negative status; a plan shorter than its header and tables or
 * inconsistent with its length, another sub_bits or rounds and NULL arrays are GTX_ERR_INVALID before anything is launched. */
int gtx_op_jpeg_entropy(gtx_ctx* ctx, const void* plan, size_t bytes, int sub_bits, int rounds, void* record, size_t capacity,
                        size_t* record_bytes, int* status, int* rounds_used);
/* Timing of what replaces cv2.VideoCapture.read(), extract.py:146, on the GPU entropy route: plan[0, bytes) is uploaded once, then the
 * entropy chain and the two pixel kernels run `reps` times (1..10000) on the context's stream with events around each part, after
 * one untimed pass. ms[0] = the entropy chain, ms[1] = the two pixel kernels, mean milliseconds per frame; *status and *rounds_used
 * as gtx_op_jpeg_entropy reports them for the last pass. tools/jpeg_time.py. */
int gtx_jpeg_entropy_ms(gtx_ctx* ctx, const void* plan, size_t bytes, int sub_bits, int rounds, int reps, float ms[2], int* status, int* rounds_used);
/* Replaces cv2.VideoCapture.read(), extract.py:146, for a feeder of kind 2: gpu != 0 puts the feeder on the GPU entropy route (its
 * reader threads write plans, the copy stream runs the entropy chain in front of the two pixel kernels, gtx_feeder_next looks at
 * the batch's status words and has gtx_jpeg_parse decode every frame whose status is not 0), gpu == 0 back on the host route.
 * Valid on a feeder of kind 2 that has no source yet; GTX_ERR_INVALID with a message for NULL, another kind or an opened feeder. */
int gtx_feeder_set_jpeg_entropy(gtx_feeder* f, int gpu);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (book-keeping): frames of a kind-2 feeder delivered so far (counted when
 * gtx_feeder_next hands their batch out, so the three add up to the frames delivered) whose entropy decode ran out[0] on the GPU,
 * out[1] on the host because gtx_jpeg_plan handed them back (or their plan did not fit the slot), out[2] on the host after a GPU
 * status. On the host route all three stay 0. */
int gtx_feeder_jpeg_stats(gtx_feeder* f, int64_t out[3]);

/* JPEG frame source, the restart-interval route (opt-in): frames that carry a DRI segment, decoded one lane per restart interval
 * (csrc/jpeg_restart.hip). At every RSTn the stream is byte aligned, the DC predictors are zero and the MCU index is known, so
 * the intervals need nothing from each other. The host keeps the header walk and removes the byte stuffing and the markers (the
 * "interval plan", csrc/jpeg_parse.hpp: header, quantisers, tables, the start of every interval, the clean stream); the GPU
 * produces the packed record, byte for byte what gtx_jpeg_parse writes for the same picture. A frame the kernel cannot vouch
 * for gets a non-zero status and is decoded by gtx_jpeg_parse, so which frames decode and what an error says does not depend on
 * the route. */
/* Replaces cv2.VideoCapture.read(), extract.py:146 (sizing): bytes of the largest interval plan a decodable h x w frame can need;
 * 0 for a size outside 1..16384. */
size_t gtx_jpeg_plan_intervals_bound(int h, int w);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (the host half of the restart-interval route): bytes[0, n) -> the interval plan
 * in out[0, capacity) (4-byte aligned; NULL with capacity 0 asks for the size). Returns 0 (written), 1 (capacity < *needed), 3 (the
 * frame has no restart interval: *needed is 0, nothing is written) or the negative status and message gtx_jpeg_parse gives for the
 * same frame: its header rules, and where a restart marker is missing or out of sequence its scan's. h, w, ncomp, hs, vs as
 * gtx_jpeg_parse. */
int gtx_jpeg_plan_intervals(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs, void* out, size_t capacity,
                            size_t* needed);
/* Kernel hook of the restart-interval decoder (tests/test_jpeg_restart_gpu.py; no product use): uploads one interval plan (host
 * memory, as gtx_jpeg_plan_intervals wrote it), runs the chain and copies the record at its real length into record[0, capacity)
 * (4-byte aligned). *status: 0 or 1 (invalid: *record_bytes is 0 and nothing is copied; gtx_jpeg_parse says what is wrong with
 * the frame). Returns 0, 1 (capacity < *record_bytes: nothing copied) or a negative status; a plan jpeg::check_plan_intervals
 * refuses is GTX_ERR_INVALID before any launch. */
int gtx_op_jpeg_restart(gtx_ctx* ctx, const void* plan, size_t bytes, void* record, size_t capacity, size_t* record_bytes, int* status);
/* Timing of what replaces cv2.VideoCapture.read(), extract.py:146, on the restart-interval route: `copies` copies of one interval
 * plan (1..64, a feeder batch) decoded `reps` times, two events around each part. ms[0] = the entropy chain (the interval launch, the
 * offset scans and the compactions), ms[1] = the two pixel kernels, mean milliseconds per frame. *status: the first copy's.
 * tools/jpeg_time.py. */
int gtx_jpeg_restart_ms(gtx_ctx* ctx, const void* plan, size_t bytes, int copies, int reps, float ms[2], int* status);
/* Replaces cv2.VideoCapture.read(), extract.py:146, for a feeder of kind 2: on != 0 sends every frame that has a restart interval
 * down the restart-interval route, whichever way gtx_feeder_set_jpeg_entropy sends the others (the two switches are independent; a
 * frame without a restart interval goes where it goes without this switch). The restart frames of a batch share one interval
 * launch. A frame whose status is not 0 is decoded again by gtx_jpeg_parse when gtx_feeder_next hands its batch out; one whose
 * plan does not fit its slot, or that gtx_jpeg_plan_intervals refuses, is decoded by gtx_jpeg_parse on its reader thread. Valid on a
 * feeder of kind 2 that has no source yet; GTX_ERR_INVALID with a message for NULL, another kind or an opened feeder. */
int gtx_feeder_set_jpeg_restart(gtx_feeder* f, int on);
/* Replaces cv2.VideoCapture.read(), extract.py:146 (book-keeping): frames of a kind-2 feeder delivered so far that out[0] the
 * restart-interval route decoded, out[1] it handed back to a reader thread (the plan did not fit the slot, or was refused),
 * out[2] gtx_jpeg_parse decoded again after a GPU status. None of them is counted by gtx_feeder_jpeg_stats. All 0 with the
 * switch off. */
int gtx_feeder_jpeg_restart_stats(gtx_feeder* f, int64_t out[3]);

/* JPEG frame sink: cv2.VideoWriter.write() (geotrax/visualize.py:298) for Motion-JPEG output, the decode above run backwards.
 * The GPU turns a packed BGR frame in HBM into the same packed record (csrc/jpeg_parse.hpp) with libjpeg's default integer
 * arithmetic (jccolor.c's 16-bit tables, h2v2 downsampling with its alternating bias, the slow-integer forward DCT, jcdctmgr.c's
 * divide, the Annex K quantisation tables scaled by jpeg_quality_scaling): the coefficients Pillow / cv2.imwrite write for the
 * same pixels. The host Huffman-codes the record with the Annex K.3 tables into a baseline JFIF file. */
typedef struct gtx_jpeg_enc gtx_jpeg_enc;
/* Replaces cv2.VideoWriter(...), visualize.py:131 (its encoder state): one encoder for h x w frames at `quality` (1..100, libjpeg's
 * scale) and `subsampling` (0 = 4:4:4, 2 = 4:2:0: libjpeg-turbo's numbers). A size outside 1..16384, another quality or
 * subsampling is GTX_ERR_INVALID before anything is allocated or launched. */
int gtx_jpeg_enc_create(gtx_ctx* ctx, int h, int w, int quality, int subsampling, gtx_jpeg_enc** out);
void gtx_jpeg_enc_destroy(gtx_jpeg_enc* enc);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (the pixel half): enqueues colour conversion + downsampling, forward DCT +
 * quantisation, the prefix sum of the block lengths and the compaction for the BGR u8 [h][w][3] frame at bgr_dptr on the
 * context's stream and returns without waiting. The frame is read on that stream: whatever overwrites it must be ordered behind
 * this call there. One frame per encoder may be in flight (GTX_ERR_INVALID otherwise): keep a ring of encoders to overlap. */
int gtx_jpeg_enc_submit_dev(gtx_jpeg_enc* enc, const void* bgr_dptr);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (the hand-over to the host): waits for the submitted frame, reads the closing
 * offset and copies the record at its real length into record[0, capacity) (4-byte aligned). *bytes receives that length.
 * Returns 0 (record filled), 1 (capacity < *bytes: nothing was copied, the frame stays collectable) or a negative status. */
int gtx_jpeg_enc_collect(gtx_jpeg_enc* enc, void* record, size_t capacity, size_t* bytes);
/* Timing of what replaces cv2.VideoWriter.write(), visualize.py:298: milliseconds of the launches of the frame collected last
 * (two events around the chain). tools/jpeg_encode_time.py. */
int gtx_jpeg_enc_last_ms(gtx_jpeg_enc* enc, float* ms);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (the entropy-coding half; host only, no context): record[0, bytes) (4-byte
 * aligned, from gtx_jpeg_enc_collect or gtx_jpeg_parse: grayscale, 4:4:4, 4:2:2 or 4:2:0) -> a baseline JFIF file in
 * out[0, capacity): SOI, APP0, DQT, SOF0, DHT (Annex K.3), SOS, the scan, EOI. The record is checked first (a damaged one, a
 * quantiser above 255 or a coefficient the Annex K.3 tables cannot code is GTX_ERR_INVALID). *n receives the file's size.
 * Returns 0 (written), 1 (capacity < *n: nothing outside out[0, capacity) was touched) or a negative status. */
int gtx_jpeg_emit(const void* record, size_t bytes, void* out, size_t capacity, size_t* n);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (host only): gtx_jpeg_emit with restart intervals of `restart_mcus` MCUs, so
 * that the file reads back one lane per interval (gtx_feeder_set_jpeg_restart): a DRI segment and, every restart_mcus MCUs, the
 * pending byte padded with 1-bits, RSTn (0..7, wrapping) and the DC predictors reset. restart_mcus 0: gtx_jpeg_emit's bytes
 * exactly; above 65535 (what DRI holds): GTX_ERR_INVALID. Everything else as gtx_jpeg_emit. */
int gtx_jpeg_emit_restart(const void* record, size_t bytes, int restart_mcus, void* out, size_t capacity, size_t* n);
/* Replaces cv2.VideoWriter.write(), visualize.py:298, on host arrays (the operator hook the kernel tests use): uploads the BGR
 * frame, runs one encoder's chain and returns the record as gtx_jpeg_enc_collect does (0, 1 or a negative status). Sizes,
 * quality and subsampling are checked before the GPU is touched. */
int gtx_op_jpeg_encode(gtx_ctx* ctx, const uint8_t* bgr, int h, int w, int quality, int subsampling, void* record, size_t capacity, size_t* bytes);
/* The GPU entropy route: the entropy-coding half of cv2.VideoWriter.write() (geotrax/visualize.py:298) as HIP kernels
 * (csrc/jpeg_huff.hip) instead of gtx_jpeg_emit on host threads. From the dense zigzag runs the forward DCT leaves in HBM: bits
 * per block (DC prediction resolved per component in scan order), an exclusive prefix sum of the bit counts, the codes packed
 * MSB first into a zeroed bit buffer, FF bytes counted, prefix-summed and stuffed, and header + scan + EOI assembled in HBM, so
 * that one copy of the picture's real length hands over a complete file: byte for byte what gtx_jpeg_emit writes for the
 * encoder's record. Bit offsets are carried in 64 bits, so every frame size gtx_jpeg_enc_create accepts is accepted here too
 * (16384 x 16384 in 4:4:4 can need 2.1e10 bits of scan; nothing is refused for its size). */
/* Replaces cv2.VideoWriter(...), visualize.py:131 (its choice of a codec back-end): gpu != 0 puts the encoder on the GPU entropy
 * route, 0 leaves it on the host route (the default). Only before the encoder's first submit (GTX_ERR_INVALID afterwards). On
 * the GPU route gtx_jpeg_enc_submit_dev enqueues the entropy coder behind the forward DCT (the record's offset scan and
 * compaction are not launched) and still returns without waiting. */
int gtx_jpeg_enc_set_entropy(gtx_jpeg_enc* enc, int gpu);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (the hand-over to the host), on the GPU entropy route: waits for the submitted
 * frame and copies the finished JPEG at its real length into out[0, capacity). *n receives that length. Returns 0 (filled), 1
 * (capacity < *n: nothing was copied, the frame stays collectable) or a negative status; GTX_ERR_INVALID on an encoder that is
 * not on the GPU route (gtx_jpeg_enc_collect is GTX_ERR_INVALID on one that is; either way the frame stays collectable by the
 * right call), and for a frame with a coefficient the Annex K.3 tables cannot code, as gtx_jpeg_emit. */
int gtx_jpeg_enc_collect_jpeg(gtx_jpeg_enc* enc, void* out, size_t capacity, size_t* n);
/* Timing of what replaces cv2.VideoWriter.write(), visualize.py:298: milliseconds of the entropy launches alone of the frame
 * collected last (gtx_jpeg_enc_last_ms covers the whole chain, these included); 0 on the host route. tools/jpeg_encode_time.py. */
int gtx_jpeg_enc_entropy_ms(gtx_jpeg_enc* enc, float* ms);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (its output buffer): the largest picture the GPU route can produce for an
 * h x w frame over the accepted samplings -- every block 64 long at the longest codes (22 + 63 * 26 bits), doubled for stuffing,
 * plus header and EOI. 0 for a size outside 1..16384. */
size_t gtx_jpeg_picture_bound(int h, int w);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (the picture's header; host only, no context): the bytes gtx_jpeg_emit writes
 * in front of the scan for this record -- SOI, APP0, DQT, SOF0, DHT, SOS -- from the one function both entropy routes call. Only
 * the record's header and quantisers are read. Returns 0, 1 (capacity < *n) or a negative status, as gtx_jpeg_emit. */
int gtx_jpeg_header(const void* record, size_t bytes, void* out, size_t capacity, size_t* n);
/* Replaces cv2.VideoWriter.write(), visualize.py:298 (the entropy-coding half), on host arrays (the operator hook the kernel tests
 * use): record[0, bytes) as gtx_jpeg_emit takes it (grayscale, 4:4:4, 4:2:2, 4:2:0; from the encoder, the parser or hand-built) is
 * expanded to dense runs + lengths, uploaded and coded by the GPU route's kernels. out[0, capacity) receives the picture, *n its
 * length; block_bits (may be NULL) the n_blocks per-block bit counts. Returns 0, 1 (capacity < *n: out untouched) or a negative
 * status (GTX_ERR_INVALID where gtx_jpeg_emit refuses the record: out untouched). */
int gtx_op_jpeg_huff(gtx_ctx* ctx, const void* record, size_t bytes, void* out, size_t capacity, size_t* n, uint32_t* block_bits);

/* ------------------------------------------------------------------ operator level
 * Single operators of the detector, exposed so the parity tests can check every kernel
 * against oracle/ on the exact layer shapes. Host buffers in, host buffers out. */

typedef struct gtx_conv_desc {
  int dtype;               /* gtx_dtype of activations (weights/bias always given as fp32) */
  int n, h, w;             /* input batch / height / width */
  int cin, cout;
  int ksize;               /* 1 or 3 (padding = ksize/2) */
  int stride;              /* 1 or 2 */
  int act;                 /* 1 = SiLU, 0 = identity */
  int in_cstride, in_coff; /* input buffer has in_cstride channels per pixel; conv reads
                              channels [in_coff, in_coff+cin) */
  int out_cstride, out_coff;
  int has_residual;        /* y += residual (residual laid out like the output slice) */
} gtx_conv_desc;

/* ultralytics Conv.forward_fuse: act(conv2d(x, w) + b) on NHWC data.
 * x: [n,h,w,in_cstride] dtype; w_ohwi: [cout,k,k,cin] fp32; bias: [cout] fp32 or NULL;
 * residual: [n,ho,wo,cout] dtype or NULL; y: [n,ho,wo,out_cstride] dtype (only the slice is
 * written; the rest of y is copied through from the caller's buffer). */
int gtx_op_conv2d(gtx_ctx* ctx, const gtx_conv_desc* d, const void* x, const float* w_ohwi,
                  const float* bias, const void* residual, void* y);
/* Repeats the same launch `iters` times and returns the mean kernel time (ms) measured with
 * HIP events on the launch stream, plus the algorithmic FLOPs of one launch. */
int gtx_op_conv2d_time(gtx_ctx* ctx, const gtx_conv_desc* d, int iters, float* ms_per_launch,
                       double* flops);
/* One GROUPED launch of n_members convolutions (the Detect stages' form: members of different Cin and map size share one
 * kernel configuration and one grid). Arrays of n_members entries: descs, xs, ws, biases (entries or the array may be NULL)
 * and ys as in gtx_op_conv2d (no residual). ty_first / ty_count (arrays or NULL): ty_count[i] > 0 computes only the
 * 8-row output tile rows [ty_first[i], ty_first[i] + ty_count[i]) of member i; the other rows of ys[i] come back as given.
 * Fails when the members do not pick the same kernel. */
int gtx_op_conv2d_group(gtx_ctx* ctx, int n_members, const gtx_conv_desc* descs, const void* const* xs, const float* const* ws,
                        const float* const* biases, void* const* ys, const int* ty_first, const int* ty_count);
/* What gtx_op_conv2d leaves off: the second source of the neck's 1x1 layers, the plain-fp32 output and the saturation flag of the
 * split-f16x3 launches, and the stages fused into the detector's first launch. Every part is off when its pointer is NULL (out_plain,
 * ty_count, force_kc, members: when 0). The launchers' own checks decide what a kernel form accepts; a refused call launches nothing. */
typedef struct gtx_conv_fused {
  const void* x2;          /* second source [n][h/2][w/2][in2_cstride] dtype: input channels [0, c_split) are its channels */
  int in2_cstride, in2_coff, c_split; /* [in2_coff, in2_coff + c_split) upsampled 2x (nearest); [c_split, cin) come from x */
  int out_plain;           /* GTX_F32S: y is written (and handed back) as plain fp32, not through the pair format */
  int* sat;                /* out: 1 when the launch clamped a value to fp16's range on its way into the pair format */
  const float* post_w;     /* post stage: [cout][cout] OHWI weights of a 1x1 layer applied to the tile before it is stored */
  const float* post_bias;  /* [cout] or NULL */
  int post_act;
  int post_separate;       /* 1: the same two layers as two launches, the 3x3 layer's pair-format output staying in HBM between them */
  const void* front_img;   /* front stage: [n][front_h][front_w_px][4] RGB0 bytes; the layer's input is the stem applied to it */
  const float* front_w27;  /* [27][cin] as gtx_op_stem's w27 */
  const float* front_bias; /* [cin] */
  int front_h, front_w_px;
  int ty_first, ty_count;  /* as gtx_op_conv2d_group */
  int force_kc;            /* > 0: the K chunk (16 or 32) instead of the library's pick; a post or front stage pins 16 by itself */
  int members;             /* > 1: the problem is put into the group that many times (a launcher's rule on the group size) */
  int res_cstride, res_coff; /* res_cstride > 0: residual is [n][ho][wo][res_cstride] and the launch adds its channels [res_coff, res_coff + cout),
                              as the trunk's bottlenecks read a chunk of their concat buffer; 0 (with res_coff 0): residual is [n][ho][wo][cout] */
  int in_place;            /* 1 (stride 1, no other extra): x, residual (if any) and y are ONE host array [n][h][w][cs], uploaded once; the launch
                              reads, adds and writes channel slices of that one device buffer. Input and residual slices must not meet the output's */
} gtx_conv_fused;
/* gtx_op_conv2d with the extras of *f; x may be NULL under a front stage (the kernel does not read it). */
int gtx_op_conv2d_fused(gtx_ctx* ctx, const gtx_conv_desc* d, const gtx_conv_fused* f, const void* x, const float* w_ohwi,
                        const float* bias, const void* residual, void* y);
/* The stem, ultralytics' Conv(3, c0, 3, 2) + SiLU on `im / 255`: img [n][h][w][4] RGB0 bytes, w27 [27][c0] fp32 with row
 * (ky * 3 + kx) * 3 + colour, bias [c0], out [n][(h-1)/2+1][(w-1)/2+1][c0] (fp16 for GTX_F16, else fp32; GTX_F32S: the values the
 * pair format holds). GTX_F16 with packed = 0 and GTX_F32: the VALU kernel; GTX_F16 with packed = 1 and GTX_F32S: the matrix-core
 * kernels on their packed weights. c0 must be 16, 32, 48, 64, 80 or 96; h, w >= 1. */
int gtx_op_stem(gtx_ctx* ctx, int dtype, int packed, int n, int h, int w, int c0, const void* img, const float* w27,
                const float* bias, void* out);
/* yolov5.yaml's stem, ultralytics' Conv(3, c0, 6, 2, 2) + SiLU on `im / 255` (F.conv2d(x, w, b, stride=2, padding=2)): img [n][h][w][4]
 * RGB0 bytes, w108 [108][c0] fp32 with row (ky * 6 + kx) * 3 + colour, bias [c0], out [n][(h-2)/2+1][(w-2)/2+1][c0] (fp16 for GTX_F16,
 * else fp32; GTX_F32S: the values the pair format holds). GTX_F16 and GTX_F32S: the matrix-core kernels on their packed weights (K = 108
 * padded with zero taps to 112); GTX_F32: the exact-fp32 kernel. c0 must be 16, 32, 48, 64, 80 or 96; h, w >= 2. iters > 0:
 * *ms_per_launch = mean time of that many further launches (may be NULL). */
int gtx_op_stem6(gtx_ctx* ctx, int dtype, int n, int h, int w, int c0, const void* img, const float* w108, const float* bias, void* out,
                 int iters, float* ms_per_launch);
/* Host only (no GPU call): how a grouped convolution launch is cut over the 8 XCDs. n_members problems of
 * blocks[i] workgroups with cin[i] input channels each, in launch order. xcd_begin[0..8]: hardware block b takes
 * logical block xcd_begin[b & 7] + (b >> 3) and exits when that reaches xcd_begin[(b & 7) + 1]; the ranges hold equal
 * work (blocks weighted by their K depth), not equal counts. grid_blocks = 8 x the longest range. */
int gtx_op_conv_xcd_ranges(int n_members, const int* blocks, const int* cin, int xcd_begin[9], int* grid_blocks);
/* Host only (no GPU call): the kernel a convolution of this shape is given (force_kc as gtx_conv_fused's; the GTX_K32 / GTX_K32S2 switches
 * are read as every launch reads them). *form: 0 the register-staged kernel (fp16, exact fp32), 1 split-f16x3 on 32x32x16, 2 its 3x3
 * stride-1 form on 16x16x32, 3 its 3x3 stride-2 form on 16x16x32; *bn: the cout tile; *kc: the input channels per K chunk; name (may be
 * NULL): the kernel's symbol with its template arguments, cut to name_cap bytes. A shape no kernel takes is an error. */
int gtx_op_conv_config(int dtype, int ksize, int stride, int cin, int cout, int force_kc, int* form, int* bn, int* kc, char* name, int name_cap);

/* SPPF max-pool cascade (three 5x5/s1/p2 pools of ultralytics SPPF.forward): reads channels
 * [0,c) of x and writes the 5x5, 9x9 and 13x13 window maxima to channels [c,2c), [2c,3c),
 * [3c,4c) of the same NHWC buffer (cstride = 4c). */
int gtx_op_sppf_pool(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, void* x_inout);
/* nn.Upsample(scale_factor=2, mode="nearest") writing into a channel slice. */
int gtx_op_upsample2x(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, const void* x,
                      int in_cstride, int in_coff, void* y, int out_cstride, int out_coff);
/* ultralytics' Attention block (YOLO11's C2PSA) on the first n of n_alloc maps: qkv [n_alloc][h][w][in_cstride] holds heads x
 * [q 32 | k 32 | v 64] channels from in_coff; out [n][h][w][out_cstride] gets softmax(q^T k * 32^-0.5) v + pe(v) in its channels
 * [out_coff, out_coff + 64 heads) and keeps the rest. pe_w [9][64 heads] tap-major, pe_b [64 heads]. Host arrays: fp16 (GTX_F16)
 * or plain fp32 (GTX_F32; GTX_F32S: converted to the pair format on the way). form: 0 = the library's rule (the small-map kernel
 * for h w <= 64), 1 / 2 = the large- / small-map kernel whatever the size. iters > 0: *ms_per_launch = mean time of that many
 * further launches. *saturated: the launch clamped a value to fp16's range (GTX_F32S). */
int gtx_op_psa_attention(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int heads, const void* qkv, int in_cstride,
                         int in_coff, const float* pe_w, const float* pe_b, void* out, int out_cstride, int out_coff, int form,
                         int iters, float* ms_per_launch, int* saturated);
/* ultralytics' AAttn attention (YOLO12's A2C2f) on n maps: the h w positions, row-major, are the tokens, cut into `area` contiguous
 * runs of h w / area (GTX_ERR_UNSUPPORTED when h w % area != 0); a token attends to its own run only. qkv [n][h][w][in_cstride] holds
 * 96 heads channels from in_coff -- planar = 0: per head [q 32 | k 32 | v 32], heads consecutive; planar = 1: [q of every head | k of
 * every head | v of every head] --; out [n][h][w][out_cstride] gets softmax(q^T k * 32^-0.5) v in its channels [out_coff, out_coff +
 * 32 heads), head-major, and keeps the rest. Host arrays as for gtx_op_psa_attention; iters, *ms_per_launch and *saturated likewise. */
int gtx_op_area_attention(gtx_ctx* ctx, int dtype, int n, int h, int w, int heads, int area, int planar, const void* qkv,
                          int in_cstride, int in_coff, void* out, int out_cstride, int out_coff, int iters, float* ms_per_launch,
                          int* saturated);

/* Depthwise k x k convolution (k = 3, 5 or 7; stride 1 or 2; pad k / 2) + bias + activation (0 none, 1 SiLU, 2 ReLU) + optional residual
 * added after the activation: x [n][h][w][c], w [k * k][c] tap-major, bias [c], res (or NULL) and out [n][ho][wo][c], c % 8 == 0. Host
 * arrays: fp16 (GTX_F16) or plain fp32 (GTX_F32; GTX_F32S: converted to the pair format on the way). *saturated: the launch clamped a
 * value to fp16's range (GTX_F32S). Channel counts that are multiples of 32 take the LDS-tiled kernel at stride 1. */
int gtx_op_dwconv(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, int k, int stride, const void* x, const float* wt, const float* bias,
                  int act, const void* res, void* out, int* saturated);

/* YOLOv9's downsampling pools in one launch (csrc/pool_down.hpp; AConv: c_max = 0, ADown: c_avg = c_max). x [n_alloc][h][w][in_cstride] holds
 * c_avg + c_max channels from in_coff. avg [n_alloc][h][w][avg_cstride], channels [avg_coff, avg_coff + c_avg): avg_pool2d(2, 1) of the first
 * c_avg channels, stored h x w with its last row and column zero (what the stride-2 3x3 convolution behind it reads as its pad). max
 * [n_alloc][h / 2][w / 2][max_cstride], channels [max_coff, max_coff + c_max): max_pool2d(3, 2, 1) of the same average of the other c_max
 * channels (NULL when c_max = 0). The first n images run; everything else in avg and max comes back as given. h, w even and >= 2; channel
 * counts, strides and offsets multiples of 8: anything else is refused before the GPU is touched. Host arrays: fp16 (GTX_F16) or plain
 * fp32 (GTX_F32; GTX_F32S: converted to the pair format on the way). iters > 0: *ms_per_launch = mean time of that many further launches. */
int gtx_op_pool_down(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c_avg, int c_max, const void* x, int in_cstride, int in_coff,
                     void* avg, int avg_cstride, int avg_coff, void* max, int max_cstride, int max_coff, int iters, float* ms_per_launch);

/* RT-DETR's token-side kernels (csrc/rtdetr_kernels.hpp), one launcher per call, for the operator-level tests. Token tensors are plain
 * fp32 rows; map tensors are NHWC host arrays of fp16 (GTX_F16) or plain fp32 (GTX_F32; GTX_F32S: converted to the pair format on the
 * way). Every size is checked before the GPU is touched: what a launcher would refuse comes back as GTX_ERR_INVALID.
 *
 * y[M][ldy], columns [ycol, ycol + Nout) = act(x[M][K] (+ x2 for the output columns [0, x2_cols)) . w[Nout][K]^T + bias) (+ res[M][ldr]);
 * the other columns of y come back as given. x2, bias, res may be NULL. K, Nout multiples of 16; act 0 none, 2 ReLU, 3 GELU (erf);
 * x2_cols a multiple of 64, or >= Nout. */
int gtx_op_rt_linear(gtx_ctx* ctx, int M, int K, int Nout, const float* x, int ldx, const float* x2, int ldx2, int x2_cols, const float* w,
                     const float* bias, const float* res, int ldr, float* y, int ldy, int ycol, int act);
/* LayerNorm (eps 1e-5) over C channels at in_coff of rows [rows][in_cstride] into channels [out_coff, out_coff + C) of out
 * [rows][out_cstride] (the rest comes back as given). Formats: F32 -> F32 / F32S / F16, F32S -> F32S, F16 -> F16. C a multiple of 8 up
 * to 1024; strides and offsets multiples of 8. *saturated: an output was clamped to fp16's range (F32S). */
int gtx_op_rt_layernorm(gtx_ctx* ctx, int rows, int C, int in_fmt, const void* in, int in_cstride, int in_coff, int out_fmt, void* out,
                        int out_cstride, int out_coff, const float* gamma, const float* beta, int* saturated);
/* softmax(q k^T / sqrt(d)) v per image and head: qkv [n * T][ld] with q at column 0, k at C, v at 2 C; out [n * T][ldo], columns
 * [0, C) written. d = C / heads in {8, 16, 32}. form: 0 = the library's rule (d = 32 on the matrix pipe), 1 = the generic kernel. */
int gtx_op_rt_mha(gtx_ctx* ctx, int n, int T, int C, int heads, const float* qkv, int ld, float* out, int ldo, int form);
/* Query selection: idx [n][nq] = the nq anchors with the largest max-over-classes score per image, descending, ties: lower anchor
 * index first. scores: n_levels (1..3) maps [n][h][w][cstride] with the nc classes from coff; fmt GTX_F32 or GTX_F16. nq <= 1024. */
int gtx_op_rt_topk(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* scores, const int* h, const int* w, const int* cstride,
                   const int* coff, int nc, int nq, int* idx);
/* mode 0: embed [n * nq][C] = the rows of the anchors idx [n][nq] in the level maps enc, anchors [n * nq][4] their logits (+inf
 * outside (0.01, 0.99)), refer [n * nq][16] = sigmoid(delta[:, :4] + anchors) in columns 0..3, zero elsewhere. mode 1: refer (given,
 * in place) = sigmoid(delta + inverse_sigmoid(refer)); enc, idx, embed and anchors are not read. delta [n * nq][ldd]. */
int gtx_op_rt_gather_refer(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* enc, const int* h, const int* w, const int* cstride,
                           const int* coff, int C, int nq, const int* idx, const float* delta, int ldd, int mode, float* embed, float* anchors,
                           float* refer);
/* Multi-scale deformable attention sampling: value levels [n][h][w][cstride] with the layer's hd channels from coff, offaw
 * [n * nq][nh * L * npts * 3] (sampling offsets, then attention logits), refer [n * nq][16]; out [n * nq][hd]. */
int gtx_op_rt_deform(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* value, const int* h, const int* w, const int* cstride,
                     const int* coff, int hd, int nh, int npts, int nq, const float* offaw, const float* refer, float* out);
/* RTDETRPredictor.postprocess: logits [n * nq][ldl], refer [n * nq][16]; out_rows [n][max_det][6] (xyxy in frame pixels, score,
 * class; rows past out_n come back as given), out_n [n], raw [n * nq][4 + nc] or NULL. class_mask0 / 1: bit c of word c / 64 keeps
 * class c. nq <= 512, nc <= 128. */
int gtx_op_rt_post(gtx_ctx* ctx, int n, int nq, int nc, const float* logits, int ldl, const float* refer, float conf, uint64_t class_mask0,
                   uint64_t class_mask1, int frame_w, int frame_h, int max_det, float* out_rows, int* out_n, float* raw);

/* RT-DETR's map-side kernels (csrc/rtdetr_kernels.hpp), one launcher per call, for the operator-level tests
 * (tests/test_rtdetr_map_ops_gpu.py). Maps are NHWC host arrays [n_alloc][h][w][cstride] of fp16 (GTX_F16) or plain fp32 (GTX_F32; GTX_F32S:
 * converted to the pair format on the way) whose channels [coff, coff + c) the launch reads or writes; the first n of the n_alloc
 * images run. An output map is given as it is before the launch and comes back whole: everything outside the launch's own slice
 * and images as given. Refused with GTX_ERR_INVALID before the GPU is touched: NULL arrays, non-positive sizes, channel counts that
 * are not multiples of 8 (16 for stem1), strides or offsets that are not multiples of 8 (the kernels move 16- and 32-byte groups), a
 * slice that does not fit its stride. *saturated: the launch clamped a value to fp16's range (GTX_F32S).
 *
 * HGStem.stem1: out [n_alloc][H / 2][W / 2][out_cstride] = ReLU(conv 3x3 stride 2 pad 1 of img / 255 + bias); img [n_alloc][H][W][4]
 * RGB0 bytes (the fourth is not read), w27 [27][c0] with row (ky * 3 + kx) * 3 + colour, bias [c0]. H and W even, c0 % 16 == 0. */
int gtx_op_rt_stem1(gtx_ctx* ctx, int dtype, int n, int n_alloc, int H, int W, int c0, const void* img, const float* w27, const float* bias,
                    void* out, int out_cstride, int out_coff, int* saturated);
/* max_pool2d(F.pad(x, [0, 1, 0, 1]), 2, 1): out(y, x) = the maximum of the 2 x 2 window at (y, x), zeros past the right and bottom border. */
int gtx_op_rt_pool2(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, const void* in, int in_cstride, int in_coff, void* out,
                    int out_cstride, int out_coff, int* saturated);
/* gtx_op_dwconv on channel slices: x at in_coff of in_cstride, res (or NULL) at res_coff of res_cstride, out at out_coff of out_cstride;
 * bias may be NULL (zero). */
int gtx_op_rt_dwconv(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, int k, int stride, const void* x, int in_cstride, int in_coff,
                     const float* wt, const float* bias, int act, const void* res, int res_cstride, int res_coff, void* out, int out_cstride,
                     int out_coff, int* saturated);
/* Nearest 2x upsampling as RT-DETR's neck runs it: gtx_op_upsample2x's launch behind the map hooks' argument checks, on the first n of
 * n_alloc images; y [n_alloc][2 h][2 w][out_cstride]. */
int gtx_op_rt_upsample2x(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, const void* x, int in_cstride, int in_coff, void* y,
                         int out_cstride, int out_coff);
/* Map -> token rows: src [n_alloc * h * w][c] plain fp32 = the map's values and q = src + pos[row % (h w)], pos [h * w][c]. pos and q
 * are NULL together (src alone is written). The rows of the images past n come back as given. */
int gtx_op_rt_tokens_in(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, const void* in, int in_cstride, int in_coff,
                        const float* pos, float* src, float* q);
/* RTDETRDecoder._generate_anchors' valid_mask on a level's map, in place: the slice of a cell whose anchor ((x + 0.5) / w, (y + 0.5) / h,
 * 0.05 * 2^level) is not strictly inside (0.01, 0.99), compared in fp32, becomes zero bits. level 0..5. */
int gtx_op_rt_mask_invalid(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, void* m, int cstride, int coff, int level);

/* The detector's post-pass kernels (csrc/det_kernels.hpp, csrc/v10_select.hip), one launcher per call, for the operator-level tests
 * (tests/test_head_ops_gpu.py). Host arrays in, host arrays out; every size and every index is checked before the GPU is touched: what
 * a launcher would refuse, or a kernel would silently mishandle, comes back as GTX_ERR_INVALID.
 *
 * One Detect level: feat [n][h][w][cstride] (GTX_F16 or GTX_F32) with the box branch's cb channels at 0 and the class branch's cc
 * channels at cb; wb [cb][64] (the final box 1x1 convolution, transposed) and bb [64]; wc [nc][cc] and bc [nc]. The gate reads
 * wc / bc, the box decode wb / bb; what a hook does not read may be NULL. Anchors are numbered level by level, row-major. */
typedef struct gtx_head_level {
  const void* feat;
  int h, w, cstride, cb, cc;
  const float* wb;
  const float* bb;
  const float* wc;
  const float* bc;
  float stride;
} gtx_head_level;
/* The score gate: per anchor the best class (ties: the lower class) of sigmoid(wc . f + bc); kept when its score > conf and the
 * class mask has its bit. count [n]: how many passed, also above cap; cand_score / cand_anchor / cand_cls [n][cap]: the first cap
 * of them in arrival order (unwritten entries: all bits set). lvl_cap > 0: lvl_count [n][4] and lvl_list [n][4][lvl_cap] file the
 * stored entries with an index below lvl_cap under their level. cc a multiple of 8; cb and cstride multiples of 8 (F16) or 4 (F32):
 * the kernel's 16-byte loads; nc in [1, 128]; at most 4 levels. */
int gtx_op_head_gate(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, float conf, uint64_t class_mask0,
                     uint64_t class_mask1, int cap, int lvl_cap, int* count, float* cand_score, int* cand_anchor, int* cand_cls, int* lvl_count,
                     int* lvl_list);
/* DFL decode of the first min(count, cap) candidates of every image: cand_box [n][cap][4] xyxy in network pixels (entries past
 * them: all bits set). cb <= 128 and no level's cb above level 0's. */
int gtx_op_head_boxes(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int cap, const int* count, const int* cand_anchor,
                      float* cand_box);
/* The same for a Detect layer with reg_max = 1 (yolo26.yaml): wb [cb][4] and bb [4], the four outputs are the signed distances l, t,
 * r, b from the cell centre in strides; cand_box = ((x + 0.5 - l), (y + 0.5 - t), (x + 0.5 + r), (y + 0.5 + b)) * stride, no clamp. */
int gtx_op_head_boxes_r1(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int cap, const int* count, const int* cand_anchor,
                         float* cand_box);
/* One Detect level of the sparse box launch (csrc/head_sparse.hip; tests/test_head_sparse_ops_gpu.py): the Detect input map feat
 * [n][h][w][cstride] plain fp32 (converted to the pair format on the way) with the layer's cin channels at coff; w1 [c1out][3][3][cin]
 * OHWI and b1 [c1out]: cv2[l][0], alone (c1out = 64) or as the first 64 outputs of a stacked box + class layer (c1out a multiple of
 * 64: the whole stack is packed, the kernel reads its first 64-cout tile under the stack's power-of-two scale); w2 [64][3][3][64]
 * and b2 [64]: cv2[l][1]; wb [64][4 * reg_max] (the final box 1x1 convolution, transposed) and bb [4 * reg_max]. cin a multiple of
 * 32; coff and cstride multiples of 8. */
typedef struct gtx_sparse_level {
  const float* feat;
  int h, w, cstride, coff, cin, c1out;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  const float* wb;
  const float* bb;
  float stride;
} gtx_sparse_level;
/* The Detect box branch at given candidates, one launch: the two 3x3 layers + SiLU at the candidates' anchors and the box decode
 * (reg_max 16: DFL; 1: the four signed distances of gtx_op_head_boxes_r1). cand_anchor [n][cap]; lvl_count [n][4] and lvl_list
 * [n][4][lvl_cap] file entry indices under their level, as the gate does; the first min(lvl_count, lvl_cap) entries of a list are
 * computed, each must lie in [0, cap) and its anchor inside the level it is filed under. count [n] is uploaded as the launch's
 * candidate count (the kernel does not read it). cand_box [n][cap][4] xyxy in network pixels (entries no list names: all bits set);
 * *sat: 1 when a first-layer value that a candidate reads left the fp16 range. At most 4 levels. */
int gtx_op_head_sparse_box(gtx_ctx* ctx, int n, int n_levels, const gtx_sparse_level* lv, int reg_max, int cap, int lvl_cap, const int* count,
                           const int* cand_anchor, const int* lvl_count, const int* lvl_list, float* cand_box, int* sat);
/* NMS of given candidates (count [n], cand_* [n][cap]; anchors in [0, 2^20)): order score descending then anchor ascending, greedy
 * suppression at IoU > iou_thr (boxes offset by 7680 * class unless agnostic), the max_nms best only, max_det rows, scale_boxes +
 * clip to the frame. which: 0 both paths, 1 the single-workgroup kernel only (an image beyond 4096 candidates or max_det beyond 2048
 * gets out_n = 0), 2 the general kernels only (an image the single-workgroup kernel covers is left alone). nms_cap: the general
 * path's sort capacity, a multiple of 64 up to 32768. out_rows [n][max_det][6], out_n [n], out_anchor [n][max_det] are read as they
 * are before the launch and come back with only what the kernels wrote changed. */
int gtx_op_nms(gtx_ctx* ctx, int n, int cap, const int* count, const float* cand_score, const int* cand_anchor, const int* cand_cls,
               const float* cand_box, float iou_thr, int agnostic, int max_nms, int nms_cap, int max_det, int src_h, int src_w, int net_h, int net_w,
               double gain, int which, float* out_rows, int* out_n, int* out_anchor);
/* YOLOv10's two-stage top-300 cut over the gate's candidates (count [n], cand_score / cand_anchor [n][cap]): sel_count [n], sel_score /
 * sel_anchor / sel_cls [n][sel_cap] in score order (ties: the lower anchor * nc + class), lvl_count / lvl_list as the gate's when
 * lvl_cap > 0 (then >= 300); scores [n][300][nc]: the kernel's scratch, one row per anchor stage 1 kept, in no particular order, and
 * score_anchor [n][300]: the anchor of each row. sel_cap in [300, 512]. Unwritten entries: all bits set. */
int gtx_op_v10_select(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, float conf, int cap, const int* count,
                      const float* cand_score, const int* cand_anchor, int sel_cap, int lvl_cap, int* sel_count, float* sel_score, int* sel_anchor,
                      int* sel_cls, int* lvl_count, int* lvl_list, float* scores, int* score_anchor);
/* The rows of given selected entries (sel_* [n][sel_cap], sel_box [n][sel_cap][4], sel_cap <= 512): the class mask, the max_det
 * cut, scale_boxes + clip. out_rows / out_n / out_anchor as gtx_op_nms. */
int gtx_op_v10_rows(gtx_ctx* ctx, int n, int sel_cap, const int* sel_count, const float* sel_score, const int* sel_anchor, const int* sel_cls,
                    const float* sel_box, uint64_t class_mask0, uint64_t class_mask1, int max_det, int src_h, int src_w, int net_h, int net_w,
                    double gain, float* out_rows, int* out_n, int* out_anchor);
/* Appearance vectors: per image the rows [0, min(out_n, max_det)) of out [n][max_det][dim] = the c[l] channels from coff[l] at anchor
 * out_anchor [n][max_det] of its level's map [n][h][w][cstride], averaged in consecutive groups of c[l] / dim; the other rows come
 * back as given. Maps: GTX_F16, GTX_F32 or GTX_F32S (plain fp32 arrays, converted to the pair format on the way; cstride a multiple
 * of 8). At most 4 levels. */
int gtx_op_obj_feats(gtx_ctx* ctx, int dtype, int n, int n_levels, const void* const* maps, const int* h, const int* w, const int* cstride,
                     const int* coff, const int* c, int dim, int max_det, const int* out_n, const int* out_anchor, float* out);

/* Brute-force L2 2-nearest-neighbour search of unit-norm 128-d float descriptors (RootSIFT): what
 * cv2.BFMatcher(NORM_L2).knnMatch(query, train, k=2) returns inside stabilo for the orthophoto
 * registration (geotrax/utils/registration.py:59-85, matcher_name='bf'). query [nq][128], train
 * [nt][128] fp32 host arrays; idx1/idx2 = nearest / second nearest train row (-1 if absent), d1/d2
 * their L2 distances (exact fp32; the search itself runs on fp16 MFMA). iters > 0 also times the
 * device passes (ms_per_pass, for bench/roofline). */
int gtx_op_match_2nn(gtx_ctx* ctx, const float* query, int nq, const float* train, int nt,
                     int* idx1, int* idx2, float* d1, float* d2, int iters, float* ms_per_pass);

/* LetterBox + BGR->RGB + /255 (ultralytics predictor preprocess, reached from
 * extract.py:153) fused with the stabilizer's gray + resize (stabilo, extract.py:177,181).
 * frame: BGR u8 [h,w,3]. out_img: [net_h,net_w,4] dtype (RGB0). out_gray: u8
 * [gray_h,gray_w] (may be NULL). */
int gtx_op_preprocess(gtx_ctx* ctx, int dtype, const uint8_t* frame, int h, int w, int net_h,
                      int net_w, void* out_img, uint8_t* out_gray, int gray_h, int gray_w);

/* ------------------------------------------------------------------ detector
 * Stands in for ultralytics YOLO(model).predict half of model.track() -- preprocess,
 * YOLOv8 forward, decode, NMS, scale back to frame coordinates (extract.py:153,222). */

typedef struct gtx_det_config {
  int imgsz;        /* cfg ultralytics.imgsz (default.yaml:235) */
  float conf;       /* ultralytics.conf  */
  float iou;        /* ultralytics.iou   */
  int max_det;      /* ultralytics.max_det */
  int agnostic_nms; /* ultralytics.agnostic_nms */
  int half;         /* ultralytics.half: 0 = fp32 activations/MFMA, 1 = fp16 */
  int rect;         /* ultralytics.rect: 0 = pad to imgsz x imgsz, 1 = minimal stride-32 rectangle */
  int nc;           /* number of classes of the model */
  int n_classes;    /* length of classes[]; 0 = keep all (ultralytics.classes) */
  int classes[80];
  int max_batch;    /* frames per forward pass the buffers are sized for (>=1) */
  int frame_h, frame_w; /* source frame size the buffers are sized for */
  int fp32_split;   /* half == 0 only. 0: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32). 1: "split-f16x3" -- fp32
                     * activations in HBM, every conv operand split into hi + lo fp16 parts in LDS, three fp16
                     * MFMAs per product with fp32 accumulation (22 significand bits per operand; same
                     * detections as the exact path within the fp32 tolerance, ~3/16 of its matrix cost) */
  int obj_feats;    /* 1: keep an appearance vector per output box (gtx_detector_features) -- what ultralytics hands BoT-SORT under
                     * `with_reid: true, model: auto` (default.yaml:376-379; engine/predictor.py get_obj_feats): the Detect layer's
                     * three input maps, each level's channels averaged in consecutive groups down to the narrowest level's width
                     * (128 for YOLOv8s), read at the anchor the box came from */
  int arch;         /* 0: YOLOv8 (Detect head + NMS). 1: the RTDETR predictor (deformable-attention decoder, no NMS; ultralytics
                     * RTDETR, extract.py:222-225) on one of two trunks, read off the tensor names like YOLOv8-P2 is:
                     * rtdetr-l (HGNetv2, AIFI + CCFM; `model.0.stem1.*`, decoder = model.28) or yolov8-rtdetr (the YOLOv8
                     * backbone + neck, `model.0.conv.*`, decoder = model.22 on model.15 / 18 / 21). The frame is then stretched to imgsz x imgsz
                     * (RTDETRPredictor.pre_transform: scale_fill), iou / agnostic_nms / rect are not read, obj_feats must be 0; half = 1: fp16 maps and
                     * weights on the fp16 MFMA convolutions, the token side (AIFI, the decoder's queries) stays fp32;
                     * gtx_detector_raw_output returns [queries][4 + nc] = xywh normalised to the frame + class scores */
  int end2end;      /* arch 0 only. 0: Detect's cv2 / cv3 branches + NMS. 1: YOLOv10's one-to-one head (`model.23.one2one_cv2 / one2one_cv3`,
                     * ultralytics.end2end, default.yaml:250) and no NMS: per image the 300 (Detect.max_det) best (anchor, class) scores --
                     * ties: the lower flat index anchor * nc + class first --, then score > conf, classes, the max_det cut, the scale to
                     * the frame; iou / agnostic_nms are not read, obj_feats must be 0. The tensors tell the graph (yolov10.yaml: SCDown, PSA =
                     * model.10, C2fCIB, v10Detect = model.23); gtx_detector_raw_output / _raw_logits return the branch that ran */
} gtx_det_config;

int gtx_detector_create(gtx_ctx* ctx, const gtx_det_config* cfg, gtx_detector** out);
void gtx_detector_destroy(gtx_detector* det);
/* Weight hand-over, one tensor at a time, using ultralytics state_dict names of the *fused*
 * model (e.g. "model.0.conv.weight" OIHW fp32, "model.0.conv.bias"). The Python host reads the
 * safetensors file. Replaces YOLO(model=...) (extract.py:222). */
int gtx_detector_set_tensor(gtx_detector* det, const char* name, const float* data, int ndim,
                            const int64_t* shape);
/* Packs weights for the kernels, plans buffers, captures the hipGraph. */
int gtx_detector_finalize(gtx_detector* det);
/* Network input size actually used (after imgsz / rect / stride rounding). */
int gtx_detector_input_size(gtx_detector* det, int* net_h, int* net_w);

/* One frame, host BGR u8 [h,w,3] -> boxes in frame pixels, sorted by confidence (the order
 * ultralytics' NMS returns). Output arrays must hold max_det entries.
 * speed_ms[3] = preprocess, inference, postprocess -- the `results[0].speed` dict that
 * extract.py:155-156 sums. */
int gtx_detector_detect(gtx_detector* det, const uint8_t* frame_bgr, int h, int w, int* n_out,
                        float* xyxy, float* conf, int* cls, float speed_ms[3]);
/* Same, frame already resident in HBM (dptr from gtx_dev_alloc). */
int gtx_detector_detect_dev(gtx_detector* det, const void* frame_dptr, int h, int w, int* n_out,
                            float* xyxy, float* conf, int* cls, float speed_ms[3]);
/* Batched variant: nb frames resident in HBM back to back; outputs are [nb][max_det]. */
int gtx_detector_detect_batch_dev(gtx_detector* det, const void* frames_dptr, int nb, int h, int w,
                                  int* n_out, float* xyxy, float* conf, int* cls,
                                  float speed_ms[3]);
/* Asynchronous pair for pipelining: _submit_dev enqueues the whole pass for nb frames resident in
 * HBM on the context's stream and returns; _collect waits for that batch and fills the outputs
 * ([nb][max_det] arrays). One batch may be in flight per detector. While it runs the caller can
 * drive the tracker and the stabilizer (another context / stream) on the previous batch. */
int gtx_detector_submit_dev(gtx_detector* det, const void* frames_dptr, int nb, int h, int w);
int gtx_detector_collect(gtx_detector* det, int* n_out, float* xyxy, float* conf, int* cls,
                         float speed_ms[3]);
/* Device pointer of the half-resolution gray image the preprocess pass wrote for batch slot b of
 * the most recently *collected* batch (the images live in a 16-deep ring: an image stays valid until
 * fourteen more batches have been submitted after the one that follows it), or NULL. The stabilizer consumes it so the frame is read from HBM once.
 * GTX_GRAY_RING is that depth: a caller that keeps images of its own per batch beside the detector's (the engine's working gray
 * images at other downsample ratios) sizes its ring by it, so that both follow one lifetime rule. */
#define GTX_GRAY_RING 16
const void* gtx_detector_gray(gtx_detector* det, int b, int* gray_h, int* gray_w);
/* Raw head output of the last forward for parity tests: [anchors][4+nc] fp32 (xywh in network
 * pixels + sigmoid class scores), like the tensor ultralytics' Detect returns. */
int gtx_detector_raw_output(gtx_detector* det, int b, float* out, int* n_anchors);
/* Same layout, class columns hold the pre-sigmoid logits (used to calibrate synthetic weights). */
int gtx_detector_raw_logits(gtx_detector* det, int b, float* out, int* n_anchors);
/* Activation of a named layer of the last forward ("model.4" ...), NHWC fp32, for parity. Refused while a batch is in
 * flight. On the split-f16x3 path with the fused front launch (YOLOv8 n / s) "model.0.conv" and "model.1.conv" are never
 * stored by the forward pass: the call recomputes them with their stand-alone launches (same products, another summation
 * order), so those two dumps are not bit for bit what the network consumed. */
int gtx_detector_layer_output(gtx_detector* det, int b, const char* layer, float* out,
                              int* h, int* w, int* c);
/* fp32_split only. *flag = 1 when an activation of a collected pass (since the last call with clear != 0) lay beyond fp16's
 * range and was clamped to +-65504 where the split-f16x3 path stores it as a (hi, lo) fp16 pair. `half: false` promises
 * fp32's range (default.yaml:245), so gtx_detector_collect / _detect* of THAT pass re-run the batch through an exact-fp32
 * detector built from the same tensors (v_mfma_f32_32x32x2_f32; the frames must still be where the caller put them, which
 * one-batch-in-flight guarantees) and every later pass goes there; gtx_detector_fell_back reports 1 from then on. Trained,
 * BN-folded YOLOv8 weights never get there; GTX_SAT_FALLBACK=0 in the environment keeps the flag and skips the re-run. */
int gtx_detector_saturated(gtx_detector* det, int clear, int* flag);
int gtx_detector_fell_back(gtx_detector* det, int* fell_back);
/* Default fp32 path: the Detect box branch (cv2[l][0], cv2[l][1]) is evaluated at the anchors that pass the score gate only, bit
 * for bit what the dense layers give there (csrc/head_sparse.hip; GTX_SPARSE_BOX=0 builds detectors without it). on = 1 when this
 * detector does so; overflows = collected batches with more candidates per image than its buffer holds (8192), which were
 * finished by the dense layers instead (end2end = 1: the branch is evaluated at the at most 300 entries the cut keeps, so none can). */
int gtx_detector_sparse_box(gtx_detector* det, int* on, int* overflows);
/* Letterbox-padding rows (ultralytics LetterBox with `rect: false`: 420 + 420 of 1920 input rows for a 16:9 frame): an activation row
 * out of reach of the frame's rows sees the same inputs for every frame, so its value is a constant of the checkpoint. The detector
 * computes those rows once when it is created (one full pass on a blank frame over every batch slot) and its later launches
 * cover the other tile rows only; the buffers keep the constants and every result is the full launches' bit for bit
 * (csrc/detector.cpp plan_pad_skip; GTX_PAD_SKIP=0 builds detectors without it). on = 1 when rows are being skipped; skipped /
 * total = 8-row tile rows left out / launched per image and pass, summed over the convolution launches. */
int gtx_detector_pad_skip(gtx_detector* det, int* on, int* skipped, int* total);
/* gtx_det_config.obj_feats: the appearance vectors of image b of the most recently collected batch, out [n][dim] fp32 in the
 * order of its boxes (n = min(box count, cap); out may be NULL to ask for n and dim). */
int gtx_detector_features(gtx_detector* det, int b, float* out, int cap, int* n, int* dim);

/* Per-kernel-family profile of one forward pass: launches, total ms (HIP events around every
 * launch on the launch stream, graph disabled) and algorithmic FLOPs / bytes. `names` receives
 * up to cap entries of 96 chars. Feeds bench.py's roofline object.
 */
/* Live variant of the profile: after gtx_detector_trace(det, n) every n-th submitted pass carries a HIP event in
 * front of every launch of its forward graph; gtx_detector_profile(det, 0, 0, ...) then returns (and
 * clears) the per-family totals of the traced passes, i.e. kernel durations as they were inside the
 * running pipeline. n = 0 switches tracing off. */
int gtx_detector_trace(gtx_detector* det, int every_n);
int gtx_detector_profile(gtx_detector* det, int nb, int iters, int cap, char* names,
                         int* launches, float* total_ms, double* flops, double* bytes,
                         int* n_families);

/* ------------------------------------------------------------------ ReID embedder
 * A separate appearance network for `with_reid: true, model: <cls checkpoint>` (BoT-SORT, Deep OC-SORT, TrackTrack;
 * default.yaml:379, :421, :470): ultralytics' trackers/bot_sort.py ReID. Per detection, save_one_box's crop (gain 1.02, pad 10)
 * resampled as classify_transforms(imgsz) does (PIL bilinear to short side imgsz, center crop), the YOLOv8-cls or YOLO11-cls backbone
 * (model.0 - model.8, fused tensors by ultralytics state_dict names) and the global average pool of model.8: [n][dim] fp32,
 * dim = model.8's channels. The Classify head is not run. fp32_split: 1 = split-f16x3 convolutions with the detector's
 * saturation rule (a pass that clamps is re-run on the exact-fp32 kernels, and every later one; gtx_embedder_fell_back), 0 = exact
 * fp32. Added in ABI 10 without changing anything before it. */
typedef struct gtx_embedder gtx_embedder;
int gtx_embedder_create(gtx_ctx* ctx, int imgsz, int max_crops, int fp32_split, gtx_embedder** out);
void gtx_embedder_destroy(gtx_embedder* e);
int gtx_embedder_set_tensor(gtx_embedder* e, const char* name, const float* data, int ndim, const int64_t* shape);
int gtx_embedder_finalize(gtx_embedder* e);
int gtx_embedder_dim(gtx_embedder* e, int* dim);
/* frames_dptr: nb BGR u8 frames [h][w][3] back to back in HBM; counts[nb]: boxes per frame; xyxy: [sum counts][4] host, frame pixels.
 * _submit_dev enqueues the pass on the context's stream (the frames are read there, in stream order; a pass whose split-f16x3
 * convolutions saturate is re-run from the same frames inside _collect) and returns; _collect waits and writes out [n][dim]
 * (cap >= n). One pass in flight per embedder. Passes of more than max_crops boxes run in chunks of max_crops. No boxes: *n = 0,
 * nothing is launched. _embed_dev = _submit_dev + _collect. */
int gtx_embedder_submit_dev(gtx_embedder* e, const void* frames_dptr, int nb, int h, int w, const int* counts, const float* xyxy);
int gtx_embedder_collect(gtx_embedder* e, float* out, int cap, int* n);
int gtx_embedder_embed_dev(gtx_embedder* e, const void* frames_dptr, int nb, int h, int w, const int* counts, const float* xyxy,
                           float* out, int cap, int* n);
/* Debug reads of the last collected pass (crop i must lie in its last chunk): the u8 network input of crop i, out [imgsz][imgsz][4]
 * (channel slots = the network's input channels, the frame's B, G, R, then 0), and a named layer's output ("model.4",
 * "model.7.conv", ...), NHWC fp32 (out NULL: shape only). */
int gtx_embedder_crops(gtx_embedder* e, int i, uint8_t* out);
int gtx_embedder_layer_output(gtx_embedder* e, int i, const char* layer, float* out, int* h, int* w, int* c);
int gtx_embedder_saturated(gtx_embedder* e, int clear, int* flag);
int gtx_embedder_fell_back(gtx_embedder* e, int* fell_back);
/* Per-launch mean times of `iters` forward passes over n crops (the last pass's network input), names 128 chars each. */
int gtx_embedder_profile(gtx_embedder* e, int n, int iters, int cap, char* names, float* ms, double* flops, int* n_ops);
/* Host only: save_one_box's clipped crop [x1, y1, x2, y2) of each of n boxes in an h x w frame (out [n][4]). */
int gtx_reid_crop_boxes(const float* xyxy, int n, int h, int w, int* out);

/* ------------------------------------------------------------------ tracker (host, C++)
 * Stands in for the tracker callback ultralytics runs inside model.track()
 * (BYTETracker / BOTSORT.update; cfg tracker.* default.yaml:361-389). */

typedef struct gtx_tracker_config {
  int type;                /* 0 = bytetrack, 1 = botsort, 2 = ocsort (default.yaml:391-404), 3 = deepocsort: ocsort + camera-motion
                              compensation by gmc_affine + (with_reid) the appearance term (default.yaml:406-427),
                              4 = fasttrack (default.yaml:426-443): ByteTrack + the occlusion handling of the fields at the end,
                              5 = tracktrack (default.yaml:445-470): multi-cue cost + iterative assignment + track-aware initialisation */
  float track_high_thresh;
  float track_low_thresh;
  float new_track_thresh;
  int track_buffer;
  float match_thresh;
  int fuse_score;
  int frame_rate;          /* ultralytics passes 30 */
  /* OC-SORT only (type 2): tracker.ocsort.{delta_t, inertia, use_byte}; min_hits is OC-SORT's own default (3) */
  int delta_t;
  float inertia;
  int use_byte;
  int min_hits;
  /* FastTracker only (type 4): tracker.fasttrack.* of the reference's config, same names and meaning (default.yaml:436-443) */
  int reset_velocity_offset_occ;
  int reset_pos_offset_occ;
  float enlarge_bbox_occ;
  float dampen_motion_occ;
  int active_occ_to_lost_thresh;
  float occ_cover_thresh;
  int occ_reappear_window;
  float init_iou_suppress;
  /* BoT-SORT only (type 1): tracker.botsort.{with_reid, proximity_thresh, appearance_thresh} (default.yaml:376-378). with_reid = 1:
   * gtx_tracker_update_feats must be used; the cost of a pair whose boxes overlap by at least proximity_thresh becomes
   * min(IoU cost, cosine distance / 2) when the latter is <= 1 - appearance_thresh (BOTSORT.get_dists) */
  int with_reid;
  float proximity_thresh;
  float appearance_thresh;
  /* TrackTrack only (type 5): tracker.tracktrack.* of the reference's config, same names and meaning (default.yaml:453-468);
   * penalty_q is accepted and has nothing to act on (the tracker sees the detector's NMS output only) */
  float lost_match_thr;
  float iou_weight, reid_weight, conf_weight, angle_weight;
  float penalty_p, penalty_q, reduce_step;
  float tai_thr;
  int min_track_len;
  /* Deep OC-SORT (type 3) with with_reid = 1 (default.yaml:420-425; `model: auto`: gtx_detector_features through
   * gtx_tracker_update_feats): proximity_thresh / appearance_thresh gate the appearance term of the first association, and
   * alpha_fixed_emb is the base factor of the track vectors' dynamic-alpha EMA (0 = 0.95). TrackTrack (type 5) with with_reid = 1
   * replaces the second HMIoU term of its cost by the cosine distance (reid_weight, default.yaml:456). */
  float alpha_fixed_emb;
} gtx_tracker_config;

int gtx_tracker_create(const gtx_tracker_config* cfg, gtx_tracker** out);
void gtx_tracker_destroy(gtx_tracker* trk);
int gtx_tracker_reset(gtx_tracker* trk);
/* One frame of detections (xyxy, conf, cls; n entries) -> active tracks. Outputs hold up to
 * cap rows: xyxy (Kalman posterior box), track id, score, class, index of the matched
 * detection (out_det_idx; -1 for a row without one: FastTracker, type 4, keeps an occluded track in the output on its
 * prediction with its last score and class -- a caller that indexes the detections with it must test for -1). gmc_affine: optional 2x3 row-major camera-motion matrix (BoT-SORT GMC), NULL =
 * identity. Mirrors BYTETracker.update + the result rewrite in
 * ultralytics/trackers/track.py:on_predict_postprocess_end. */
int gtx_tracker_update(gtx_tracker* trk, int n, const float* xyxy, const float* conf,
                       const int* cls, const double* gmc_affine, int cap, int* n_out,
                       float* out_xyxy, int* out_id, float* out_score, int* out_cls,
                       int* out_det_idx);

/* gtx_tracker_update with one appearance vector per detection (feats [n][feat_dim] fp32, e.g. gtx_detector_features): BOTrack's
 * normalised current vector and its 0.9-EMA, used by the first association and the unconfirmed one when
 * gtx_tracker_config.with_reid is set (ultralytics/trackers/bot_sort.py). feats == NULL behaves like gtx_tracker_update. */
int gtx_tracker_update_feats(gtx_tracker* trk, int n, const float* xyxy, const float* conf, const int* cls,
                             const double* gmc_affine, const float* feats, int feat_dim, int cap, int* n_out,
                             float* out_xyxy, int* out_id, float* out_score, int* out_cls, int* out_det_idx);

/* The sequential half of a frame-sharded run (rank 0): n_recs per-frame records in clip order, each `stride`
 * doubles laid out as geotrax_amd/distributed.py::pack_frame_record writes them -- n, max_det x (x1, y1, x2, y2, conf, cls),
 * [with_gmc: valid, 2x3 camera-motion warp,] valid, h11..h33 -- go through gtx_tracker_update one after the other
 * (tracker.update on every frame, empty or not; the record's warp for BoT-SORT). rows_per_frame[f] = tracks of frame f;
 * the row_* arrays (row_cap rows) receive them back to back, as gtx_tracker_update would have returned them. */
int gtx_tracker_replay(gtx_tracker* trk, const double* recs, int n_recs, int stride, int max_det, int with_gmc,
                       int row_cap, int* rows_per_frame, float* row_xyxy, int* row_id, float* row_score,
                       int* row_cls, int* row_det_idx);

/* The trackers' assignment solver on its own (host only, no GPU): what `lap.lapjv(cost, extend_cost=True, cost_limit=L)`
 * returns for ultralytics/trackers/utils/matching.py:linear_assignment (lapx, pyproject.toml:58) when cost_limit > 0 -- a pair is
 * matched only below L, an unmatched row or column costs L/2 -- and the plain minimum-cost assignment of min(rows, cols) pairs
 * (scipy.optimize.linear_sum_assignment) when cost_limit <= 0. cost: rows x cols row-major; row_to_col[r] = column or -1;
 * col_to_row (may be NULL) the inverse. Exposed so that tests can hold the solver against scipy on its own. */
int gtx_op_linear_assignment(const float* cost, int rows, int cols, double cost_limit, int* row_to_col, int* col_to_row);

/* ------------------------------------------------------------------ stabilizer
 * Stands in for stabilo.Stabilizer as used at extract.py:139,177-187 and
 * geotrax/utils/registration.py:59-85. */

typedef struct gtx_stab_config {
  float downsample_ratio;      /* stabilo downsample_ratio (default.yaml:106): any value in (0, 1] */
  int max_features;            /* per frame; the reference frame gets ref_multiplier x */
  float ref_multiplier;
  float filter_ratio;          /* Lowe ratio */
  float ransac_threshold;      /* px, full-resolution units */
  int ransac_max_iter;
  float ransac_confidence;
  int mask_use;
  float mask_margin_ratio;
  int fast_threshold;          /* ORB fastThreshold (OpenCV default 20) */
  int n_levels;                /* ORB pyramid levels (8) */
  float scale_factor;          /* ORB pyramid scale (1.2) */
  uint32_t seed;               /* RANSAC sampling seed */
  int frame_h, frame_w;
  int clahe;                   /* stabilo clahe (default.yaml:105): cv2.createCLAHE(2.0, (8, 8)) on the working gray image */
  int affine;                  /* stabilo transformation_type (default.yaml:121): 0 = projective, 1 = affine (3-point samples,
                                  six-parameter refit; the matrix handed back is 3x3 with last row 0 0 1) */
  int filter_type;             /* stabilo filter_type (default.yaml:117): 0 = ratio (Lowe, filter_ratio), 1 = none (every query
                                  keypoint's nearest neighbour goes to the estimator) */
} gtx_stab_config;

int gtx_stabilizer_create(gtx_ctx* ctx, const gtx_stab_config* cfg, gtx_stabilizer** out);
/* The stabilizer's optional pre-processing step on its own: cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(gray)
 * (stabilo `clahe: true`, reference default.yaml:105). gray, out: u8 [h,w] on the host. */
int gtx_op_clahe(gtx_ctx* ctx, const uint8_t* gray, int h, int w, uint8_t* out);
void gtx_stabilizer_destroy(gtx_stabilizer* st);
/* Stabilizer.set_ref_frame(frame, boxes): boxes xywh [n,4] in frame pixels or NULL. */
int gtx_stabilizer_set_ref_frame(gtx_stabilizer* st, const uint8_t* frame_bgr, int h, int w,
                                 const float* boxes_xywh, int n);
/* The stabilizer's working-resolution gray image of a BGR u8 frame [h][w][3] in HBM, written to gray_dptr (gh * gw bytes, any
 * alignment) by one launch on the context's stream: cv2.cvtColor(BGR2GRAY) then cv2.resize(fx = fy = downsample_ratio,
 * INTER_LINEAR), as stabilo makes it and as gtx_stabilizer_set_ref_frame / _stabilize make it of a host frame. Any ratio in
 * (0, 1]; gh, gw must be the working size gtx_op_gray_working_size gives (h / 2, w / 2 at 0.5; h, w at 1.0; else rint(h * ratio),
 * rint(w * ratio), halves to even), anything else is GTX_ERR_INVALID. The image feeds the _gray_dev entries below of a stabilizer
 * created with the same frame size and ratio. The tap tables are made on the host once per context, frame size and working size,
 * and stay with the context: at most 16 such pairs per context (a 17th is GTX_ERR_INVALID), and the gray_resize entries of ONE
 * context must not be called from two threads at once (contexts are independent; the engine calls them from its detector stage).
 * gh, gw are passed although the library can compute them: the caller sized gray_dptr by them, and a caller whose idea of the
 * working size differs from the library's is refused here instead of having its buffer overrun. */
int gtx_op_gray_working_size(int h, int w, float ratio, int* gh, int* gw);
int gtx_op_gray_resize_dev(gtx_ctx* ctx, const void* bgr_dptr, int h, int w, float ratio, void* gray_dptr, int gh, int gw);
/* Mean milliseconds of that launch over `reps` launches between two events on the context's stream, after 3 untimed ones
 * (tools/stab_ratio_time.py). */
int gtx_op_gray_resize_ms(gtx_ctx* ctx, const void* bgr_dptr, int h, int w, float ratio, void* gray_dptr, int gh, int gw, int reps, float* ms);
/* The same on host arrays (staged, synchronous): the kernel on its own, for tests. */
int gtx_op_gray_resize(gtx_ctx* ctx, const uint8_t* bgr, int h, int w, float ratio, uint8_t* gray, int gh, int gw);
/* Same as _set_ref_frame, from a gray image of the stabilizer's working size already in HBM (gtx_detector_gray at downsample_ratio 0.5,
 * gtx_op_gray_resize_dev at any ratio). Another size is GTX_ERR_INVALID; so for the _gray_dev entries below. */
int gtx_stabilizer_set_ref_gray_dev(gtx_stabilizer* st, const void* gray_dptr, int gh, int gw,
                                    const float* boxes_xywh, int n);
/* Stabilizer.stabilize(frame, boxes) + get_cur_trans_matrix(): H maps current-frame pixels
 * to reference-frame pixels (row-major 3x3 f64). valid = 0 when no transform could be
 * estimated (the reference then gets None and skips the row, extract.py:185). stats[4] =
 * keypoints ref, keypoints cur, good matches, inliers (registration.py:83-85). */
int gtx_stabilizer_stabilize(gtx_stabilizer* st, const uint8_t* frame_bgr, int h, int w,
                             const float* boxes_xywh, int n, double H[9], int* valid,
                             int stats[4]);
int gtx_stabilizer_stabilize_gray_dev(gtx_stabilizer* st, const void* gray_dptr, int gh, int gw,
                                      const float* boxes_xywh, int n, double H[9], int* valid,
                                      int stats[4]);
/* Asynchronous pair of _stabilize_gray_dev for pipelining: _submit enqueues keypoints, matching and
 * RANSAC on the stabilizer's stream and returns; _collect waits and runs the host refit. */
int gtx_stabilizer_submit_gray_dev(gtx_stabilizer* st, const void* gray_dptr, int gh, int gw,
                                   const float* boxes_xywh, int n);
int gtx_stabilizer_collect(gtx_stabilizer* st, double H[9], int* valid, int stats[4]);
/* The features of the frame stabilized last become the reference (buffers swapped; needs ref_multiplier = 1): frame-to-frame
 * registration (gmc_method orb) without extracting every frame's features twice. */
int gtx_stabilizer_promote_cur(gtx_stabilizer* st);
/* GPU time (ms) of the last collected asynchronous pass: what the reference logs as "Average stabilization
 * time" (geotrax/extract.py:175,188,206) is the wall time of the blocking stabilo calls; here the pass runs on
 * its own stream beside the detector, so its stream-ordered duration is reported instead. */
int gtx_stabilizer_last_ms(gtx_stabilizer* st, float* ms);
/* Keypoints / descriptors of the last processed image (for parity tests): xy in full-res
 * pixels, level, angle bin, 32-byte descriptors. */
int gtx_stabilizer_keypoints(gtx_stabilizer* st, int which /*0 ref, 1 cur*/, int cap, int* n,
                             float* xy, int* level, int* angle_bin, uint8_t* desc);
/* Good matches of the last stabilize call: pairs (cur index, ref index) and Hamming distance. */
int gtx_stabilizer_matches(gtx_stabilizer* st, int cap, int* n, int* cur_idx, int* ref_idx,
                           int* dist);

/* Read-backs of the LAST extract pass, for the per-kernel tests. _keep_pass(st, 1) makes every later pass keep its level plan and a
 * copy of its candidate counters (one small device copy per pass; off by default, and then nothing is kept). `which` (0 ref, 1 cur)
 * must name the set the last pass filled: the pyramid and the candidate lists are shared by both.
 * _level: pyramid level i as h x w bytes (out may be NULL: sizes only; cap = room in out).
 * _candidates: level i after FAST, 3x3 non-maximum suppression and the mask: n (pix = y * w + x, FAST score) pairs in no particular
 * order (pix / score may be NULL: counts only; cap = room in each); n_elig = how many of them stage 1 handed to the Harris ranking,
 * n_kp = keypoints kept on the level, n_dropped = candidates that found their sub-list full (0: the lists hold every possible corner). */
int gtx_stabilizer_keep_pass(gtx_stabilizer* st, int on);
int gtx_stabilizer_level(gtx_stabilizer* st, int which, int i, int* h, int* w, uint8_t* out, int64_t cap);
int gtx_stabilizer_candidates(gtx_stabilizer* st, int which, int i, int cap, int* n, int* pix, int* score, int* n_elig, int* n_kp,
                              int* n_dropped);

/* The stabilizer's matcher on its own: ONE launch of its kernel, shaped as the stabilizer shapes it (a grid over slots_q x slots_t
 * keypoint slots, slots_* >= n*, of which nq / nt are filled). desc_q [nq][32], desc_t [nt][32] u8, xy_q [nq][2], xy_t [nt][2] f32.
 * Per query: best_idx (lowest index among equals; -1 when nt = 0), best_d, second_d (2^30 where there is none). Then the Lowe test
 * best_d < ratio * second_d in fp32 (keep_all: every query with a neighbour), survivors compacted in query order: m_q, m_t, m_d
 * [nq], m_pts [nq][4] = (xy_q, xy_t), n_match. Entries past n_match: all bits set. The kernel's ticket word lives with the context
 * and is written by the host once, before the first call: every later call relies on the launch before it having re-armed it. */
int gtx_op_orb_match(gtx_ctx* ctx, const uint8_t* desc_q, int nq, int slots_q, const uint8_t* desc_t, int nt, int slots_t, float ratio,
                     int keep_all, const float* xy_q, const float* xy_t, int* best_idx, int* best_d, int* second_d, int* m_q, int* m_t,
                     int* m_d, float* m_pts, int* n_match);
/* The stabilizer's RANSAC kernel on its own, without the host refit: n_hyp <= 65536 hypotheses (4-point homographies, or 3-point
 * affine maps) sampled by the counter hash of (seed, hypothesis, draw) from pts [n][4] = (x, y) -> (z, w), scored by the truncated
 * squared error in units of 1/1024 px^2. best = the winner's index (lowest cost, then lowest index; -1: no hypothesis could be
 * made), cost = its integer cost, H = its matrix as sampled (all zero when best = -1). The state words live with the context like
 * the matcher's ticket. */
int gtx_op_orb_ransac(gtx_ctx* ctx, const float* pts, int n, uint32_t seed, int n_hyp, int frame_w, int frame_h, float thr, int affine,
                      int* best, int64_t* cost, double H[9]);

/* The steered-BRIEF sampling table the descriptor kernel uses: [256 orientation bins][256
 * tests][ax, ay, bx, by] int8 = 262144 bytes. `st` may be NULL (the table does not depend on the
 * object and needs no device). The oracle generates its own table from the published recipe and
 * the parity tests compare the two. */
int gtx_stabilizer_pattern(gtx_stabilizer* st, int8_t* out);

/* ------------------------------------------------------------------ global motion compensation
 * BoT-SORT's camera-motion estimate, gmc_method 'sparseOptFlow' (geotrax/cfg/default.yaml:374), the
 * per-frame step ultralytics' BOTSORT.update runs before association (reached from extract.py:153):
 * Shi-Tomasi corners of the half-resolution gray frame, pyramidal Lucas-Kanade against the previous
 * frame, RANSAC similarity. A = row-major 2x3 f64 mapping previous-frame to current-frame pixels
 * (full resolution); feed it to gtx_tracker_update(gmc). Identity (valid = 0) on the first frame or
 * when fewer than 5 corners could be tracked. stats = {corners of the previous frame, tracked, inliers}. */
typedef struct gtx_gmc gtx_gmc;
int gtx_gmc_create(gtx_ctx* ctx, int frame_h, int frame_w, int seed, gtx_gmc** out);
void gtx_gmc_destroy(gtx_gmc* g);
int gtx_gmc_reset(gtx_gmc* g);
int gtx_gmc_apply(gtx_gmc* g, const uint8_t* frame_bgr, int h, int w, double A[6], int* valid, int stats[3]);
/* Asynchronous pair on the half-resolution gray image the detector left in HBM (gtx_detector_gray).
 * Up to 64 frames may be submitted ahead (the image is copied at submit); _collect returns their warps
 * in submission order. */
int gtx_gmc_submit_gray_dev(gtx_gmc* g, const void* gray_dptr, int gray_h, int gray_w);
/* The next submitted frame opens a new sequence (identity warp); unlike _reset, frames may still be in flight. */
int gtx_gmc_restart(gtx_gmc* g);
/* The same for a full BGR u8 frame [h][w][3] in HBM (gray + 2x2 mean first). restart != 0: the frame opens a new
 * sequence -- its own warp is the identity and the next submitted frame is compensated against it. A rank of the
 * frame-sharded run hands the GMC the frame that precedes its batch in the clip this way. */
int gtx_gmc_submit_frame_dev(gtx_gmc* g, const void* frame_bgr_dptr, int h, int w, int restart);
int gtx_gmc_collect(gtx_gmc* g, double A[6], int* valid, int stats[3]);
/* Parity hook: which 0 = corners of the last frame, 1 = corners of the frame before, 2 = where LK put
 * those in the last frame (+ status). xy in half-resolution pixels. */
int gtx_gmc_points(gtx_gmc* g, int which, int cap, int* n, float* xy, int* status);
/* The corner step's record of the last submitted frame: counts = {3x3 local maxima found (equal neighbours all count), stored in
 * the candidate list (the list holds every pixel inside the border, so: the same number), gathered into LDS for the final sort (at
 * most 4032 once the list is longer than 4096), radix passes that narrowed the gather (0 on ordinary frames)}. */
int gtx_gmc_counts(gtx_gmc* g, int counts[4]);

/* The method's kernels one launcher at a time on host arrays, each launch shaped as gtx_gmc_submit_* shapes it; sizes and
 * coordinates are checked before the GPU is touched.
 * _corners: response + nms + select on a gray image [h][w] u8 (16..8192 a side) -> n <= 1000 corners, strongest first, equal
 * responses by larger pixel index first, xy [n][2] f32 (cap = room in xy, at least 1000), counts as gtx_gmc_counts.
 * _lk: the three pyramid reductions of both images, then the Lucas-Kanade kernel on n <= 1000 caller-given points pts [n][2] f32
 * (fractional, anywhere inside the image) -> next [n][2] f32, status [n] (1 = tracked).
 * _ransac: the hypothesis kernel and its arg-max on pairs [n][4] f32 = (p.x, p.y, q.x, q.y), n <= 1024 -> count [512] per hypothesis
 * (-1: none could be made), the winner's index (most inliers, lowest index among equals; -1: none), best_count (-1: none) and
 * model = (a, b, tx, ty) of [a -b tx; b a ty] as sampled (the identity when there is no winner). No host refit. */
int gtx_op_gmc_corners(gtx_ctx* ctx, const uint8_t* gray, int h, int w, int cap, int* n, float* xy, int counts[4]);
int gtx_op_gmc_lk(gtx_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int h, int w, const float* pts, int n, float* next, int* status);
int gtx_op_gmc_ransac(gtx_ctx* ctx, const float* pairs, int n, uint32_t seed, int* best_count, int* winner, double model[4], int* count);

/* ------------------------------------------------------------------ global motion compensation, method 'orb'
 * `gmc_method: orb` (geotrax/cfg/default.yaml:374,419,467): ultralytics' GMC.apply_features on ORB keypoints of the half-resolution
 * gray image -- the stabilizer's FAST / Harris / steered-BRIEF kernels (max_features <= 1024 per frame), Hamming 2-NN of the current
 * frame's descriptors (query) against the previous frame's, Lowe ratio 0.9, apply_features' two spatial filters, then the
 * partial-affine RANSAC of gtx_op_estimate_affine_partial -- as ONE chain on the context's stream per submitted frame, like
 * gtx_gmc_*: up to 64 frames may be submitted ahead (the image is copied at submit), _collect waits for the oldest, refits on the
 * host and returns the warps in submission order. A, valid as gtx_gmc_*; stats = {keypoints of the previous frame, pairs kept,
 * inliers}. _reset / _restart / _submit_frame_dev(restart) follow gtx_gmc_*. _submit_gray takes the gray image from host memory. */
typedef struct gtx_fgmc gtx_fgmc;
int gtx_fgmc_create(gtx_ctx* ctx, int frame_h, int frame_w, int max_features, int seed, gtx_fgmc** out);
void gtx_fgmc_destroy(gtx_fgmc* g);
int gtx_fgmc_reset(gtx_fgmc* g);
int gtx_fgmc_restart(gtx_fgmc* g);
int gtx_fgmc_submit_gray_dev(gtx_fgmc* g, const void* gray_dptr, int gray_h, int gray_w);
int gtx_fgmc_submit_gray(gtx_fgmc* g, const uint8_t* gray, int gray_h, int gray_w);
int gtx_fgmc_submit_frame_dev(gtx_fgmc* g, const void* frame_bgr_dptr, int h, int w, int restart);
int gtx_fgmc_collect(gtx_fgmc* g, double A[6], int* valid, int stats[3]);
/* Parity hooks (nothing may be in flight). _pairs: the pairs the filters kept for the frame collected last, rows (prev.x, prev.y,
 * cur.x, cur.y) in full-resolution pixels, in match order. _matches: what the filters were given for the frame submitted last --
 * per keypoint of that frame the index of the nearest keypoint of the frame before (-1: none) and the two smallest Hamming
 * distances, plus both frames' keypoint positions; *n_q = *n_t = 0 when the frame opened a sequence. */
int gtx_fgmc_pairs(gtx_fgmc* g, int cap, int* n, float* pairs4);
int gtx_fgmc_matches(gtx_fgmc* g, int cap, int* n_q, int* n_t, int* best_idx, int* best_d, int* second_d, float* q_xy, float* t_xy);
/* The gray + 2x2-mean pass of gtx_gmc_submit_frame_dev on its own: BGR u8 [h][w][3] in HBM -> u8 [h / 2][w / 2] in HBM (the bytes
 * the detector's gray image holds), enqueued on the context's stream. */
int gtx_gray_half_dev(gtx_ctx* ctx, const void* frame_bgr_dptr, int h, int w, void* gray_dptr);

/* ------------------------------------------------------------------ camera-motion compensation, method 'ecc'
 * `gmc_method: ecc` (geotrax/cfg/default.yaml:374,419,467): ultralytics' GMC.apply_ecc, i.e. cv2.findTransformECC(first frame,
 * current frame, MOTION_EUCLIDEAN, (EPS | COUNT, max_iters = 5000, eps = 1e-6), None, 1) on cvtColor(BGR2GRAY) -> GaussianBlur(3x3, 1.5)
 * -> resize(1/2). As upstream, every frame is registered against the FIRST frame since the last reset, and A -- row-major 2x3,
 * float32 values -- is in half-resolution pixels (upstream does not scale the translation back for this method). Identity for
 * the first frame. info = {iterations run, status: 0 finished, 1 NaN correlation, 2 the correlation was about to be minimised
 * (both raise cv2.error upstream, which the caller there catches and keeps the matrix as the failed call left it: so does A)}.
 * _submit_dev prepares the frame's image at once on `producer`'s stream (the context whose stream wrote the frame, e.g. the
 * detector's; NULL = the object's own) into a 32-deep ring; _collect returns the frames in submission order. */
typedef struct gtx_ecc gtx_ecc;
int gtx_ecc_create(gtx_ctx* ctx, int frame_h, int frame_w, int max_iters, double eps, gtx_ecc** out);
void gtx_ecc_destroy(gtx_ecc* e);
int gtx_ecc_reset(gtx_ecc* e);
/* replace != 0: every collected frame becomes the template of the next one (frame-to-frame warps). Default 0 = upstream's behaviour. */
int gtx_ecc_replace_template(gtx_ecc* e, int replace);
/* exact != 0 (default): warpAffine's bilinear samples as OpenCV >= 4.11 takes them (source position in floating point); 0: as through
 * 4.10 (fixed point, rounded to 1/32 pixel; many fits then never meet eps and run to max_iters -- oracle/ecc_ref.py). */
int gtx_ecc_exact_positions(gtx_ecc* e, int exact);
int gtx_ecc_submit(gtx_ecc* e, const uint8_t* frame_bgr, int h, int w);
int gtx_ecc_submit_dev(gtx_ecc* e, gtx_ctx* producer, const void* frame_bgr_dptr, int h, int w);
int gtx_ecc_collect(gtx_ecc* e, double A[6], int info[2], double* rho);
/* Parity hook: which 0 = the prepared image of the frame collected last, 1 = the template; out [h / 2][w / 2] float32 */
int gtx_ecc_image(gtx_ecc* e, int which, float* out);
/* The method's kernels on host arrays, each launch shaped as gtx_ecc_submit / _collect shape it; sizes and pointers are checked
 * before the GPU is touched.
 * _prepare: the prepare kernel on a BGR u8 frame [H][W][3], H, W >= 8 (as gtx_ecc_create) -> out [H / 2][W / 2] f32.
 * _iterate: the gradient kernel on img, then exactly ONE round of stats, stats-finish, accum and update on template and image
 * [h][w] f32 (2..8192 a side), starting from the state given: map [6] (row-major 2x3, finite, entries within 1e6), exact (0 / 1),
 * rho_in, last_rho_in, eps > 0, 0 <= iter_in < max_iters, status_in (0..2) and done_in (0 / 1; 1: every kernel of the round
 * returns at once). Out: gx, gy [h][w] f32; partial_stats, partial_accum [512][13] f64 -- the partial-sum buffer as it stands after
 * the stats kernel (columns 0..4 of each block's row: count, sum and sum of squares of the sample, the same of the template; the
 * other columns still hold the 0xFF bytes the whole buffer is filled with before that launch) and after the accum kernel (Hessian 6,
 * image projection 3, template projection 3, correlation); map_out [6]; state_i = {iter, status, done}; state_d = {rho, last_rho,
 * n, img_norm, tmp_norm}; means = {img_mean, tmp_mean}, the float32 values the masked subtraction uses. */
int gtx_op_ecc_prepare(gtx_ctx* ctx, const uint8_t* frame_bgr, int H, int W, float* out);
int gtx_op_ecc_iterate(gtx_ctx* ctx, const float* tmpl, const float* img, int h, int w, const float map[6], int exact, double rho_in,
                       double last_rho_in, double eps, int iter_in, int max_iters, int status_in, int done_in, float* gx, float* gy,
                       double* partial_stats, double* partial_accum, float map_out[6], int state_i[3], double state_d[5], float means[2]);

/* ------------------------------------------------------------------ registration (once per video)
 * Replaces estimate_homography() of geotrax/utils/registration.py:21-95 -- stabilo.Stabilizer with
 * detector_name='rsift', matcher_name='bf', filter_type='ratio', projective model, no mask, no
 * downsampling -- as used by the georeference stage for frame <-> master frame <-> orthophoto
 * (SURVEY.md K11). RootSIFT keypoints/descriptors on the GPU, brute-force L2 2-NN on MFMA, Lowe
 * ratio, robust homography (MSAC hypotheses + IRLS refit; the reference uses MAGSAC++). */
typedef struct gtx_reg_config {
  int max_features;         /* SIFT nfeatures: strongest responses kept (reference default 250000) */
  float filter_ratio;       /* Lowe ratio (reference default 0.55) */
  float ransac_threshold;   /* reprojection threshold in destination pixels (3.0) */
  int ransac_max_iter;      /* hypotheses (10000; clamped to [256, 16384]) */
  float ransac_confidence;  /* accepted for interface parity; the hypothesis count is fixed */
  float rsift_eps;          /* RootSIFT L1-normalisation epsilon (1e-8); negative: plain SIFT descriptors (stabilo `detector_name: sift`) */
  int seed;
} gtx_reg_config;
/* src/dst: BGR u8 [h][w][3] host images. H (row-major 3x3 f64) maps src pixels to dst pixels;
 * stats = {n_src_keypoints, n_dst_keypoints, n_good_matches, n_inliers}; *valid = 0 when no model
 * was found (the reference then retries with half the features, registration.py:87-91);
 * timings_ms (may be NULL) = {detect+describe both images, matching, ratio filter, robust fit}. */
int gtx_register_images(gtx_ctx* ctx, const gtx_reg_config* cfg, const uint8_t* src_bgr, int src_h,
                        int src_w, const uint8_t* dst_bgr, int dst_h, int dst_w, double H[9],
                        int* valid, int stats[4], float timings_ms[4]);
/* The detector stage on its own (cv2.SIFT_create(nfeatures, enable_precise_upscale=True)
 * .detectAndCompute + stabilo's RootSIFT conversion when root != 0), for parity tests: keypoints as
 * rows {x, y, size, angle, response} + the packed octave word, descriptors [n][128] fp32. */
typedef struct gtx_sift gtx_sift;
int gtx_sift_create(gtx_ctx* ctx, int max_h, int max_w, gtx_sift** out);
void gtx_sift_destroy(gtx_sift* s);
int gtx_sift_detect(gtx_sift* s, const uint8_t* image_bgr, int h, int w, int max_features, int root,
                    float root_eps, int cap, int* n, float* kp5, int* octave, float* desc);
/* GPU milliseconds of the stages of the last detect call (HIP events on the context's stream): out[0] upload + gray + Gaussian / DoG
 * pyramid, out[1] extrema + refinement + orientation (with the host round trips for their counters), out[2] descriptors; out[3] = the
 * pixel count of the doubled base image (the pyramid is 11 x 4/3 fp32 images of that size: what a roofline of the stage is priced on). */
int gtx_sift_stage_ms(gtx_sift* s, float out[4]);
/* Gaussian (kind 0) or DoG (kind 1) image of the last detect call, [h][w] fp32. */
int gtx_sift_pyramid(gtx_sift* s, int kind, int octave, int layer, int cap, float* out, int* h, int* w,
                     int* n_octaves);

/* The SIFT kernels one stage at a time on host arrays (images [h][w] fp32, 1..4096 a side), each launched as gtx_sift_detect
 * launches it over a one-octave pyramid table; sizes, and every record field a kernel turns into an address, are checked before the
 * GPU is touched. `octave` (0..15) is the octave the images belong to: records carry it, and positions and sizes scale with 2^octave.
 * Records are rows of 32-bit words:
 *   candidate [4] i32 = (octave, layer, row, column);
 *   refined  [13]     = f32 (x, y, size, response), i32 (octave word, octave, layer, row, column), the candidate it came from;
 *   oriented [13]     = f32 (x, y, size, angle, response), i32 (octave word, octave, layer), the candidate, i32 orientation bin;
 *   final    [8]      = f64 ori (360 - angle, degrees), f32 (px, py: octave-local position; scl), i32 (octave = 0, layer, 0).
 * _blur: dst = Gaussian(src, sigma) with radius ((int)rint(8 sigma + 1) | 1) / 2 <= 16 (a larger one is an error), dog (may be NULL) =
 *   dst - src. form 0: as the pyramid dispatches it (a compile-time instance for radii 5, 6, 8, 10, 13, else the generic tile kernel),
 *   1: the generic tile kernel, 2: row pass, column pass and subtraction pass. All three give the same bits.
 * _extrema: dog5 = the octave's five DoG layers [5][h][w]; the three layer passes. *count = every candidate, the first min(count, cap)
 *   entries of cand are stored candidates in no particular order (which ones, when count > cap, depends on the run).
 * _refine: n candidates of layers 1..3 inside the border of 5 -> *count accepted records in out [n][13], in no particular order.
 * _orient: n refined records (layer 0..5 all read gauss_layer) -> *count peaks, the first min(count, cap) stored in out [cap][13];
 *   hist [n][36] = the smoothed orientation histogram of every input record.
 * _describe: n final records -> desc [n][128]: 0..255 integers, or their RootSIFT form sqrt(d / (sum(d) + root_eps)) when root != 0. */
int gtx_op_sift_blur(gtx_ctx* ctx, const float* src, int h, int w, double sigma, int form, float* dst, float* dog);
int gtx_op_sift_extrema(gtx_ctx* ctx, const float* dog5, int h, int w, int octave, int cap, int* count, int* cand);
int gtx_op_sift_refine(gtx_ctx* ctx, const float* dog5, int h, int w, int octave, const int* cand, int n, int* count, void* out);
int gtx_op_sift_orient(gtx_ctx* ctx, const float* gauss_layer, int h, int w, int octave, const void* refined, int n, int cap, int* count,
                       void* out, float* hist);
int gtx_op_sift_describe(gtx_ctx* ctx, const float* gauss_layer, int h, int w, const void* finals, int n, int root, float root_eps,
                         float* desc);

/* The selection stage of the stream-ordered extraction on host arrays: of n oriented records (rows of 13 words, above; any order) the
 * max_features strongest stay -- response descending, equal responses by key (octave, layer, row, column, orientation bin)
 * ascending; fewer than max_features: all of them -- and come out in ascending key order with the kept keypoints whose
 * working-resolution position, rounded as (int)(v + 0.5f), lies inside one of the n_rects inclusive rectangles rects [n_rects][4] i32
 * (x1, y1, x2, y2) dropped (cv2: the mask is applied after retainBest). *count = keypoints left; finals [count][8] words (the final
 * record above), xy [count][2], kp5 [count][5] and octave [count] as gtx_sift_detect reports them (each may be NULL). The result
 * depends on the set of records only. Refused before the GPU is touched: n outside [0, 2^20], max_features outside [1, 65536], more
 * than 1024 rectangles, a response that is not finite or is negative, an octave outside 0..15, a layer outside 0..7, a row or column
 * outside [0, 2^20), a bin outside 0..255, two records with one key. */
int gtx_op_sift_select(gtx_ctx* ctx, const void* oriented, int n, int max_features, const int* rects, int n_rects, int* count, void* finals,
                       float* xy, float* kp5, int* octave);

/* ------------------------------------------------------------------ stabilizer, detector_name sift / rsift
 * stabilo.Stabilizer with `detector_name: sift | rsift`, matcher bf, filter_type ratio, projective model, on the detector's
 * half-resolution gray image in HBM: the kernels of gtx_register_images as one stream-ordered chain. The reference frame's features
 * are extracted once (_set_ref_gray_dev; lround(max_features * ref_multiplier) of them, as the ORB stabilizer plans its reference
 * set). _submit_gray_dev enqueues extraction (every count stays in HBM), fp16 descriptors, the L2 2-NN search, Lowe's ratio with the
 * pair list, and the RANSAC launch on the context's stream and returns without waiting; _collect waits, checks the counters (a stage
 * that counted more than its list holds: GTX_ERR_UNSUPPORTED, as gtx_sift_detect) and runs the robust refit on the host.
 * H maps current to reference pixels OF THE WORKING IMAGE (row-major 3x3 f64); the caller conjugates it with the downsample
 * ratio. stats[4] = keypoints ref, keypoints cur, pairs after the ratio test, inliers; valid = 0 (not an error) with fewer than 1
 * current keypoint, 2 reference keypoints or 4 pairs, or when no model is found. The vehicle mask (boxes xywh [n][4] in frame pixels
 * grown by mask_margin_ratio, scaled by downsample_ratio, floor / ceil, clipped, inclusive -- the ORB path's rule) drops kept
 * keypoints after the strongest max_features were chosen, as cv2's detectAndCompute(image, mask) does. For the same images, seed,
 * threshold and max_iter the pairs, stats and H are those of gtx_register_images, provided the matcher splits the reference set alike
 * for max_features query rows (this chain) and for the frame's own keypoint count (gtx_register_images): always so below 2048
 * reference keypoints. At most 1024 rectangles are masked; boxes beyond them are ignored. Each object keeps one Gaussian / DoG pyramid in
 * HBM (about 59 bytes per pixel of the doubled working image); _create fails with the sizes when that does not fit. */
typedef struct gtx_sift_stab_config {
  int work_h, work_w;          /* the working (gray) image */
  int max_features;            /* per frame; the reference frame gets lround(max_features * ref_multiplier) */
  float ref_multiplier;
  int root;                    /* 1: RootSIFT descriptors (rsift), 0: plain SIFT */
  float rsift_eps;             /* RootSIFT L1-normalisation epsilon (1e-8) */
  float filter_ratio;          /* Lowe ratio */
  float ransac_threshold;      /* px of the working image */
  int ransac_max_iter;         /* hypotheses, clamped to [256, 16384] */
  float ransac_confidence;     /* accepted for interface parity; the hypothesis count is fixed */
  int mask_use;
  float mask_margin_ratio;
  float downsample_ratio;      /* frame pixels -> working pixels (scales the boxes of the mask) */
  uint32_t seed;               /* RANSAC sampling seed */
} gtx_sift_stab_config;
typedef struct gtx_sift_stab gtx_sift_stab;
int gtx_sift_stab_create(gtx_ctx* ctx, const gtx_sift_stab_config* cfg, gtx_sift_stab** out);
void gtx_sift_stab_destroy(gtx_sift_stab* st);
int gtx_sift_stab_set_ref_gray_dev(gtx_sift_stab* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n);
int gtx_sift_stab_submit_gray_dev(gtx_sift_stab* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n);
int gtx_sift_stab_collect(gtx_sift_stab* st, double H[9], int* valid, int stats[4]);
/* _submit_gray_dev + _collect */
int gtx_sift_stab_stabilize_gray_dev(gtx_sift_stab* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n, double H[9],
                                     int* valid, int stats[4]);
/* GPU time (ms, stream-ordered events) of the last collected pass: extraction -> matching -> RANSAC */
int gtx_sift_stab_last_ms(gtx_sift_stab* st, float* ms);
/* Keypoints of the reference (which 0) or of the last collected frame (1, until the next submit), rows as gtx_sift_detect's. */
int gtx_sift_stab_keypoints(gtx_sift_stab* st, int which, int cap, int* n, float* kp5, int* octave, float* desc);
/* The pair list of the last collected frame: pts [n][4] = (x_cur, y_cur, x_ref, y_ref) in query order. */
int gtx_sift_stab_pairs(gtx_sift_stab* st, int cap, int* n, float* pts);
/* The extraction's counters of the last collected frame: extrema candidates, refined, oriented, keypoints kept. */
int gtx_sift_stab_counters(gtx_sift_stab* st, int out[4]);

/* Stabilizer.transform_cur_boxes(): maps the 4 corners of each xywh box through H and
 * returns the axis-aligned bounding rectangle as xywh (rule pinned on the reference's golden
 * output). Pure host arithmetic, f64 inside, f32 out. */
int gtx_warp_boxes(const double H[9], const float* xywh_in, int n, float* xywh_out);

/* cv2.perspectiveTransform on N points (georeference.py:599-605), f64. */
int gtx_perspective_points(const double H[9], const double* x, const double* y, int n,
                           double* ox, double* oy);

/* cv2.estimateAffinePartial2D(prev, cur, RANSAC) as ultralytics' GMC calls it for `gmc_method: orb` / `sift` (default.yaml:374):
 * the 4-parameter similarity p -> q of n matched points ([n][2] float32 each), A row-major 2x3 f64; *valid = 0 when no model
 * exists (fewer than two distinct points). Host code (a few hundred matches); no device needed. */
int gtx_op_estimate_affine_partial(const float* p_xy, const float* q_xy, int n, unsigned seed, double A[6], int* valid, int* n_inliers);

/* The host half of every robust homography here (the ORB and SIFT stabilizers, gtx_register_images): the IRLS refit of a RANSAC
 * winner H0 (row-major 3x3 f64 as gtx_op_orb_ransac returns it, any scale) on n point pairs (x, y) -> (z, w), [n][4] float32, of a
 * frame_w x frame_h frame; thr in pixels; affine = 1 keeps h31 = h32 = 0. *valid = 1: H (h33 = 1) and *n_inliers, the pairs within
 * thr of it. *valid = 0: no model (too few pairs near H0, or too few inliers), H untouched. Host code; no device needed. */
int gtx_op_homography_refit(const float* pairs, int n, int frame_w, int frame_h, double thr, int affine, const double H0[9], double H[9],
                            int* valid, int* n_inliers);

/* The georeference stage's per-row transform chain in one HIP pass (replaces
 * geotrax/georeference.py:173-177 = apply_homography :599-605 -> ortho2geo :608-615 -> geo2local :618-628, where the
 * reference reprojects through pyproj): frame pixel -H-> orthophoto pixel -affine-> lat/lon (deg)
 * -transverse Mercator (Krueger series, 6th order)-> metres. f64. x, y and every non-NULL output are host arrays of n. */
typedef struct gtx_georef_chain {
  double H[9];            /* frame (stabilized) pixel -> orthophoto pixel */
  double ortho[6];        /* lng0, lat0, dlng, dlat, skew_x, skew_y (georeference.py:608-615) */
  int projected;          /* 0: stop at lat/lon; east/north are not written */
  double semi_major, flattening;            /* ellipsoid of the target CRS */
  double lon0_deg, k0;                      /* central meridian, scale on it */
  double false_easting, false_northing;     /* false_northing includes -k0 * (meridian arc to the latitude of origin) */
} gtx_georef_chain;
int gtx_op_georef_points(gtx_ctx* ctx, const gtx_georef_chain* chain, const double* x, const double* y, int n,
                         double* ortho_x, double* ortho_y, double* lat, double* lon, double* east, double* north);

/* Every per-row and per-track column of the georeference stage in HBM (replaces, opt-in, the host functions
 * geotrax/georeference.py:651-799 and :458-479 run after the chain above): one upload of the track table, the chain of
 * gtx_op_georef_points on (x, y), then calculate_visibility, convert_dimensions, compute_kinematics (gap filling, speed,
 * Gaussian / Savitzky-Golay smoothing, acceleration) and the road-section / lane lookup, one download. f64 throughout.
 *   The table is in file order. The host hands in the grouping it has from the integer columns (the plan):
 *   order[n]            the rows sorted by track id, stable (np.argsort(track_ids, kind="stable"))
 *   seg[n_tracks + 1]   the tracks' bounds in `order`: 0 = seg[0] < seg[1] < ... < seg[n_tracks] = n
 *   n_used[n_tracks]    per track, its rows with visibility && is_interpolated == 0 (the rows the kinematics use)
 *   exp_off[n_tracks+1] per track, where its gap-filled series starts in the scratch buffers: a track of fewer than 3 used rows
 *                       takes no room, any other 1 + the sum over its consecutive used rows of (gap > 1 ? gap : 1), gap = the
 *                       difference of their frame numbers (a repeated frame number adds one point).
 *   The hook refuses, before any launch, a plan that cannot belong to n rows; the kernels count every track's used rows and
 *   series length themselves and write nothing for a track whose plan entry differs: the call then fails (GTX_ERR_INVALID).
 *   bbox_unstab: [n][4] x_c, y_c, w, h of the un-stabilized box; veh_dim_px: [n][2] length, width in pixels (NaN = unknown);
 *   frame_num: [n]; is_interpolated: [n] or NULL (every row is a detection).
 *   quads: [n_quads][8] x, y of four corners in any winding (the segmentation file's columns 3..10); n_quads <= 512.
 *   weights: [n_weights] the smoothing filter in correlation order, n_weights odd, <= 4095; cfg->boundary says how a series is
 *   continued past its ends: 0 = half-sample symmetric reflection, repeated as often as needed (scipy 'reflect': the Gaussian),
 *   1 = the end value (scipy 'nearest': Savitzky-Golay). The sum runs in scipy.ndimage.correlate1d's order -- centre tap, then
 *   for k = radius .. 1 (in[i-k] + in[i+k]) * weights[radius-k] when the weights are symmetric to DBL_EPSILON, else the last tap
 *   then the others left to right -- one rounding per operation, whatever the launch shape.
 *   Outputs, host arrays of n, any may be NULL: the six columns of gtx_op_georef_points, visibility (0 / 1), length_m / width_m
 *   (the track's first row in file order decides; NaN in, NaN out), speed (m/s * conversion_factor) / accel (NaN on rows the
 *   kinematics do not use, on a track's first used row, and for accel on its second), quad (index of the first quad in file
 *   order that strictly contains the row's orthophoto point, -1 for none; points on an edge or a vertex are outside).
 * n == 0 is success. chain->projected must be 1. */
typedef struct gtx_georef_tracks_cfg {
  int frame_h, frame_w;            /* frame_size of calculate_visibility / convert_dimensions */
  int visibility_margin;
  double fps, conversion_factor;   /* compute_kinematics: speed = |dp| * fps * conversion_factor, accel = dv * fps */
  int boundary;                    /* 0 reflect, 1 nearest */
  int n_tracks;
} gtx_georef_tracks_cfg;
#define GTX_GEOREF_TRACKS_MS 12
int gtx_op_georef_tracks(gtx_ctx* ctx, const gtx_georef_chain* chain, const gtx_georef_tracks_cfg* cfg, const double* x,
                         const double* y, const double* bbox_unstab, const double* veh_dim_px, const int32_t* frame_num,
                         const int32_t* is_interpolated, int n, const int32_t* order, const int32_t* seg, const int32_t* n_used,
                         const int64_t* exp_off, const double* quads, int n_quads, const double* weights, int n_weights,
                         double* ortho_x, double* ortho_y, double* lat, double* lon, double* east, double* north,
                         uint8_t* visibility, double* length_m, double* width_m, double* speed, double* accel, int32_t* quad);
/* Event times of this thread's last gtx_op_georef_tracks, milliseconds: [0] the chain, [1] visibility, [2] dimensions,
 * [3] use-mask + compaction + series positions, [4] gap fill, [5] speed, [6] correlate, [7] acceleration + scatter, [8] lanes,
 * [9] the uploads, [10] the downloads, [11] the nine kernels together. */
int gtx_georef_tracks_ms(float ms[GTX_GEOREF_TRACKS_MS]);

/* cv2.warpPerspective(frame, H, (w,h)) with bilinear sampling and constant-0 border
 * (visualize.py:289). BGR u8 in/out, host buffers. */
int gtx_warp_frame(gtx_ctx* ctx, const uint8_t* src_bgr, int h, int w, const double H[9],
                   uint8_t* dst_bgr);
/* Same, both images resident in HBM (dptrs from gtx_dev_alloc, distinct buffers); enqueued on the
 * context's stream, returns without waiting (gtx_ctx_synchronize / a later call on the stream orders it). */
int gtx_warp_frame_dev(gtx_ctx* ctx, const void* src_dptr, int h, int w, const double H[9], void* dst_dptr);
/* The inverse of H that the two calls above hand their kernel (the adjugate over the determinant, f64), row-major. Host arithmetic,
 * no context and no device. GTX_ERR_INVALID, with inv left as it was, when the determinant is zero or not finite -- the
 * matrices gtx_warp_frame refuses as singular. */
int gtx_op_invert3x3(const double H[9], double inv[9]);

/* ------------------------------------------------------------------ drawing (for the visualize stage)
 *
 * Replaces the cv2 drawing calls of annotate_frame / draw_oriented_box / _draw_dashed_poly (visualize.py:747-783, :807, :934-939):
 * cv2.rectangle (outline and filled), cv2.line, cv2.polylines, cv2.circle and cv2.putText become one list of primitives that one
 * kernel paints into the BGR u8 frame [h][w][3] where it lies in HBM. A primitive is eight int32 -- kind, x0, y0, x1, y1, p0, p1,
 * bgr (b | g << 8 | r << 16) -- kind 0 FILL (corners inclusive), 1 SEGMENT (endpoints, p0 = thickness, anti-aliased, round caps),
 * 2 RING (centre, x1 = radius, p0 = thickness), 3 GLYPH (cell top-left, x1 y1 = cell size, p0 = byte offset into the coverage
 * atlas, p1 = row pitch); applied in index order. The pixel rule is specified in geotrax_amd/draw.py, whose numpy twin the kernel
 * equals byte for byte; its differences from OpenCV's rasteriser are listed in DESIGN.md.
 *
 * Every record is checked before anything is launched: kind in 0..3; x0, y0, x1, y1 in [-32768, 32767]; thickness >= 1 (SEGMENT,
 * RING); radius >= 0; a GLYPH with x1, y1, p1 > 0, p0 >= 0 and p0 + (y1 - 1) p1 + x1 <= atlas_bytes; n <= max_prims. A violation is
 * GTX_ERR_INVALID with the record's index in the message, and nothing is drawn: no record is ever dropped. */
typedef struct gtx_drawer gtx_drawer;
/* A drawer for h x w frames (1..16384 each side) and lists of up to max_prims (1..2^20) primitives. The atlas (atlas_bytes bytes of
 * coverage, 0..255; NULL with 0 bytes when no GLYPH is drawn) is uploaded once, here. */
int gtx_drawer_create(gtx_ctx* ctx, int h, int w, int max_prims, const void* atlas, size_t atlas_bytes, gtx_drawer** out);
/* Waits for the context's stream (a queued upload may still read the pinned ring): destroy a drawer before its context. */
void gtx_drawer_destroy(gtx_drawer* drawer);
/* Validates the list, stages it (a ring of four pinned buffers: the call returns before the launch before it has read its list),
 * enqueues upload and kernel on the context's stream and returns without waiting. prims may be reused at once. n = 0 launches
 * nothing. frame_dptr: h * w * 3 bytes in HBM, painted in place. */
int gtx_drawer_draw_dev(gtx_drawer* drawer, void* frame_dptr, const int32_t* prims, int n);
/* Milliseconds of the last gtx_drawer_draw_dev's launch, between two events (waits for it); 0 when that call launched nothing.
 * The list's upload, enqueued ahead of the launch on the same stream, is outside the two events. tools/visualize_time.py. */
int gtx_drawer_last_ms(gtx_drawer* drawer, float* ms);
/* Operator hook (tests/test_draw_ops_gpu.py): a host frame, painted in place through one drawer. Sizes and records are checked
 * before the GPU is touched. */
int gtx_op_draw(gtx_ctx* ctx, uint8_t* bgr, int h, int w, const int32_t* prims, int n, const void* atlas, size_t atlas_bytes);

/* ------------------------------------------------------------------ trajectory maps (for the plot stage)
 *
 * Replaces plt.imshow(ortho) + plt.plot / plt.scatter per vehicle + plt.savefig of plot_trajectories_in_given_coordinates
 * (plot.py:419-488, :740-756) for the pictures that have a pixel hot path: the orthophoto (or a white page) becomes a BGR u8
 * canvas in HBM, semi-transparent strokes and discs are blended into it through per-tile lists, and the canvas goes to the JPEG
 * encoder where it lies. A primitive is 32 bytes: float x0, y0, x1, y1, width; int32 bgr (b | g << 8 | r << 16), alpha (1..256,
 * in 1/256 steps), poly. Coordinates are canvas pixels (a pixel's centre is at its integer coordinates), finite, in
 * [-32768, 32767], a record spanning at most 2048 pixels per axis; width 0.25..64 pixels; a zero-length record is the disc of
 * diameter `width`. A run of consecutive records with one `poly` is a polyline (same width, bgr and alpha throughout): a pixel
 * takes the maximum coverage over its records and is blended once, polylines in list order. The pixel rule is specified in
 * geotrax_amd/plot_draw.py, whose numpy twin the kernels (csrc/plot_draw.hip) equal byte for byte. Every bad size, count, width,
 * alpha or coordinate is GTX_ERR_INVALID with the record's index in the message, before anything is uploaded; no primitive is
 * ever dropped (the tile lists are sized exactly from a counting pass). */
typedef struct gtx_plot_canvas gtx_plot_canvas;
/* image: h x w x channels u8 on the host (1 = gray, 3 = RGB, 4 = RGBA, alpha ignored), reduced by the exact box average of
 * factor k (1..256; round half up; edge blocks over the pixels they have) into a BGR canvas of ceil(h / k) x ceil(w / k), which
 * must be within 1..16384 per side: what gtx_jpeg_enc_create accepts. Waits for the upload and the reduce launch. */
int gtx_plot_canvas_create(gtx_ctx* ctx, const uint8_t* image, int h, int w, int channels, int k, gtx_plot_canvas** out);
void gtx_plot_canvas_destroy(gtx_plot_canvas* canvas);
int gtx_plot_canvas_size(gtx_plot_canvas* canvas, int* h, int* w);
/* Blends n records (up to 2^22) into the canvas: count -> prefix sum -> fill -> per-tile sort -> paint on the context's stream. */
int gtx_plot_canvas_draw(gtx_plot_canvas* canvas, const void* prims, int n);
/* The canvas, h x w x 3 BGR, to the host. */
int gtx_plot_canvas_read(gtx_plot_canvas* canvas, uint8_t* bgr);
/* The canvas's device pointer (packed BGR, pitch 3 w), for gtx_jpeg_enc_submit_dev on the same context. Owned by the canvas. */
int gtx_plot_canvas_dptr(gtx_plot_canvas* canvas, void** dptr);
/* out[0..8): milliseconds between events of the creation's upload and reduce and of the last draw's binning launches and paint
 * launch; that draw's tile count, list entries in all, longest list, primitive count. tools/plot_time.py. */
int gtx_plot_canvas_stats(gtx_plot_canvas* canvas, double out[8]);
/* Operator hook (tests/test_plot_draw_gpu.py): buf holds a canvas of h rows of `pitch` bytes (pitch >= 3 w; the first 3 w bytes
 * of a row are its pixels) within buf_bytes >= (h - 1) pitch + 3 w bytes; the whole buffer is uploaded, painted and downloaded,
 * and every byte that is not a pixel comes back as it went in. Sizes and records are checked before the GPU is touched. */
int gtx_op_plot_draw(gtx_ctx* ctx, uint8_t* buf, size_t buf_bytes, int h, int w, size_t pitch, const void* prims, int n);
/* Operator hook: the reduce launch alone on a host image; bgr_out: ceil(h / k) x ceil(w / k) x 3. */
int gtx_op_plot_reduce(gtx_ctx* ctx, const uint8_t* image, int h, int w, int channels, int k, uint8_t* bgr_out);

/* ------------------------------------------------------------------ result files (host code, no GPU work)
 *
 * The text tables the two stages end with, byte for byte as the reference writes them, formatted on a few threads.
 * gtx_write_table_f32 / _f64 replace np.savetxt(path, table, fmt='%.<precision>g', delimiter=',') of save_results
 * (geotrax/extract.py:497-516: the tracks with '%g' = precision 6 on float32 rows, the transforms with '%.16g' on float64 rows;
 * save_homography's '%.20g' line, georeference.py:879-889). data: rows x cols, row-major. n_threads <= 0: up to 8.
 * gtx_write_csv replaces pandas.DataFrame.to_csv(path, index=False) for the georeferenced table (georeference.py:802-877):
 * header_line = the column names joined by commas; kinds[c]: 0 = int64 column, 1 = float64 column written as repr(float)
 * (shortest round-trip digits, NaN = empty cell), 2 = int32 codes into categories[c][0 .. n_categories[c]) (strings already
 * quoted as a CSV cell needs; a negative code = missing = empty cell; categories / n_categories may be NULL without such columns).
 * columns[c]: `rows` values of the column's kind. */
int gtx_write_table_f32(const char* path, const float* data, int64_t rows, int cols, int precision, int n_threads);
int gtx_write_table_f64(const char* path, const double* data, int64_t rows, int cols, int precision, int n_threads);
int gtx_write_csv(const char* path, const char* header_line, int n_cols, const int* kinds, const void* const* columns,
                  const char* const* const* categories, const int* n_categories, int64_t rows, int n_threads);
/* The per-row walk of estimate_vehicle_dimensions (geotrax/extract.py:433-452) for every track of a table in one call (host code).
 * xc, yc: the observations' centres, float32, the rows of track t at [start[t], start[t+1]). is_anchor[row] = 1 where the reference's
 * loop finds the observation at least `radius` pixels from the current anchor (and makes it the next one); step_dx / step_dy[row]:
 * that step, for the caller's azimuth test. The same float32 operation sequence as the NumPy scalars of the reference (csrc/table_writer.cpp). */
int gtx_track_anchor_walk(const float* xc, const float* yc, const int64_t* start, int n_tracks, float radius,
                          uint8_t* is_anchor, float* step_dx, float* step_dy);

#ifdef __cplusplus
}
#endif
#endif /* GTX_H_ */
