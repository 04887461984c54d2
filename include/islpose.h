/*
 * islpose.h — C ABI of libislpose.so, the MI355X (gfx950) OpenPose keypoint engine.
 *
 * Drop-in boundary for the reference's hot path
 * (sunilsarolkarcds/ISL-SignLanguage-Translation):
 *
 *   module seam  : bodypose_25_model / bodypose_model / handpose_model .forward
 *                  (src/model.py:179-207, 302-329, 394-407), weights loaded through
 *                  util.transfer (src/util.py:35-44)          -> isl_net_create,
 *                  isl_net_set_param, isl_net_forward
 *   frame seam   : Body.__call__ (src/body.py:39-235)         -> isl_net_preprocess
 *                  (one call per pyramid scale) + isl_net_run + isl_body_post
 *                  Hand.__call__ (src/hand.py:24-74)          -> isl_net_preprocess /
 *                  isl_net_preprocess_crops + isl_net_run + isl_hand_post
 *
 * Conventions
 *   - every function returns 0 (ISL_OK) or a negative ISL_E_* code and records a
 *     message retrievable with isl_last_error() (thread-local);
 *   - device pointers are plain HIP device addresses; the caller owns every I/O
 *     buffer, the library owns the weights and an activation arena per net;
 *   - `stream` is a hipStream_t (NULL = default stream); work is stream-ordered,
 *     no function synchronises the device except where noted;
 *   - one isl_net per device; not thread-safe without external locking.
 */
#ifndef ISLPOSE_H
#define ISLPOSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISL_ABI_VERSION 1

enum isl_kind { ISL_BODY25 = 0, ISL_COCO = 1, ISL_HAND = 2 };

enum isl_status {
  ISL_OK = 0,
  ISL_E_ARG = -1,       /* bad argument / shape                                  */
  ISL_E_PARAM = -2,     /* unknown or missing parameter name (Python: KeyError)  */
  ISL_E_HIP = -3,       /* HIP runtime error                                     */
  ISL_E_CAPACITY = -4,  /* a fixed-capacity result buffer overflowed             */
  ISL_E_STATE = -5,     /* call sequence error (e.g. forward before all params)  */
  ISL_E_INDEX = -6,     /* reference IndexError (3-way subset match, body.py:196)*/
  ISL_E_RANGE = -7      /* split-fp16 conv: an activation reached |x| >= 65504   */
};

/* Convolution arithmetic (all fp32-accurate; not in the reference, which runs
 * torch's fp32 conv):
 *   ISL_ALGO_X3     every conv on the FP16 matrix cores with 3-term operand
 *                   splitting (x*w = xh*wh + xh*wl + xl*wh, fp32 accumulate) --
 *                   the default;
 *   ISL_ALGO_WINO   3x3 convs as Winograd F(2x2,3x3) on the FP32 matrix cores;
 *   ISL_ALGO_DIRECT every conv as a direct implicit GEMM on the FP32 matrix cores. */
enum isl_algo { ISL_ALGO_X3 = 0, ISL_ALGO_WINO = 1, ISL_ALGO_DIRECT = 2 };

/* Precision of the ISL_ALGO_X3 convolutions (not in the reference):
 *   ISL_PREC_FP32   three fp16 products per multiply-add, fp32-accurate -- the default,
 *                   bit for bit what the library computed before this switch existed;
 *   ISL_PREC_FP16   one fp16 product per multiply-add: the activations are rounded to
 *                   fp16 (round to nearest even) once when a kernel stages them, the
 *                   filters are packed as their fp16 roundings (the same per-layer 2^s),
 *                   accumulation stays fp32 in the same K order.  A third of the matrix
 *                   work and half the operand bytes; the maps carry ~2e-3 of their
 *                   maximum in error instead of ~2e-6.  Opt-in.
 * Under ISL_ALGO_WINO / ISL_ALGO_DIRECT the value is stored and has no effect. */
enum isl_precision { ISL_PREC_FP32 = 0, ISL_PREC_FP16 = 1 };

/* Storage of the activations between the ISL_ALGO_X3 convolutions of ISL_PREC_FP16 (not in the
 * reference; a switch of its own, orthogonal to the precision):
 *   ISL_ACT_FP32   every arena buffer holds fp32 -- the default, nothing changes;
 *   ISL_ACT_FP16   the arena buffers between the convs hold fp16: a one-term kernel rounds
 *                  every activation to fp16 (round to nearest even) before its first use
 *                  anyway, so its producer stores that rounding -- the same value whoever
 *                  computes it, and max-pooling commutes with a monotone rounding -- and the
 *                  net's outputs are the same bits as with ISL_ACT_FP32.  The net input and
 *                  the net outputs stay fp32 (the outputs unrounded, in buffers of their own);
 *                  the activation buffers and the epilogues' writes halve.  Opt-in.
 * The value takes effect only under ISL_ALGO_X3 with ISL_PREC_FP16; otherwise it is stored and
 * has no effect.  It is all or nothing per run: where any conv of a run would take a kernel
 * without an fp16-storage form (K ranges across blocks -- split-K and the wave-range kernel --
 * i.e. the small latency-bound grids, and the 96-pixel small 7x7 tiles), the whole run uses an
 * fp32 arena exactly as under ISL_ACT_FP32 (isl_net_act_storage_active then reports 0). */
enum isl_act_storage { ISL_ACT_FP32 = 0, ISL_ACT_FP16 = 1 };

typedef struct isl_net isl_net;

int isl_abi_version(void);
const char* isl_last_error(void);

/* ---- module seam --------------------------------------------------------- */

/* Replaces `bodypose_25_model()` / `bodypose_model()` / `handpose_model()`
 * construction (src/model.py:66,210,331) on `device`. */
int isl_net_create(int kind, int device, isl_net** out);
int isl_net_destroy(isl_net* net);

/* Parameter table in caffe naming (the keys of the flat weight dict that
 * util.transfer maps onto state_dict, src/util.py:35-44). */
int isl_net_param_count(const isl_net* net);
int isl_net_param_info(const isl_net* net, int index, const char** name, int64_t* numel);

/* Copy one parameter from host memory (float32, the caffe/torch layout:
 * OIHW for conv weights).  Unknown name or wrong numel -> ISL_E_PARAM.
 * Weights are repacked for the MFMA kernels once all are present. */
int isl_net_set_param(isl_net* net, const char* caffe_name, const float* host, int64_t numel);

/* Replaces `model.forward(x)`: x is float32 NCHW [n,3,h,w] on the device.
 * body25/coco: out0 = PAF [n,npaf,h/8,w/8], out1 = heat [n,njoint,h/8,w/8];
 * hand: out0 = heat [n,22,h/8,w/8], out1 must be NULL.  (floor-mode pooling.)
 * With ISL_ALGO_X3 an element of x outside the fp16 split range -- !(|x| < 65504): too large,
 * +-inf or NaN -- raises the range flag (isl_net_check), like a conv output that leaves it. */
int isl_net_forward(isl_net* net, const float* d_x_nchw, int n, int h, int w,
                    float* d_out0, float* d_out1, void* stream);

/* ---- frame seam ---------------------------------------------------------- */

/* Pre-processing of Body/Hand.__call__ for one scale (body.py:53-56):
 * frames uint8 [n,H,W,3] (BGR, device) -> cv2.resize(INTER_CUBIC, fx=fy=scale)
 * -> padRightDownCorner(stride 8, 128) -> float32/256 - 0.5, written straight
 * into the net's input buffer.  Returns the padded net size in *net_h, *net_w. */
int isl_net_preprocess(isl_net* net, const uint8_t* d_frames, int n, int H, int W,
                       double scale, int* net_h, int* net_w, void* stream);

/* A square (or any) sub-image of frame `frame`: pixels [y, y+h) x [x, x+w). */
typedef struct {
  int32_t frame, x, y, w, h;
} isl_crop;

/* Pre-processing of a batch of crops (Hand.__call__ on oriImg[y:y+h, x:x+w],
 * src/hand.py:33-41; demo.py:36): crop i is resized by fx = fy =
 * scale_times_box / h_i (the reference's `scale = x * boxsize / oriImg.shape[0]`)
 * with OpenCV's INTER_CUBIC on the crop as its own image (borders replicated
 * at the crop's edges), padded and normalised into slot i of the net input.
 * Every crop must resize to the same padded net size (true for the hand
 * pyramid: round(s * 368) for every crop width); otherwise ISL_E_ARG. */
int isl_net_preprocess_crops(isl_net* net, const uint8_t* d_frames, int n_frames, int H, int W,
                             const isl_crop* crops, int n_crops, double scale_times_box, int* net_h,
                             int* net_w, void* stream);

/* isl_net_preprocess_crops with a left-right mirror per crop (not in the reference, which
 * inherited pytorch-openpose's omission of OpenPose's left-hand mirroring): `flip` is a host
 * array of n_crops flags, NULL for none.  Crop i with flip[i] != 0 fills its slot with exactly
 * what isl_net_preprocess_crops writes for the contiguous image crop[:, ::-1]: the kernel reads
 * source column sw - 1 - xi for every column xi it would read, in the cubic and the identity
 * path; everything indexed by the output column (OpenCV's SIMD-body / scalar-tail split of a
 * row, the pad) is unchanged -- the resize of a mirrored crop is not the mirror of the resize.
 * flip == NULL is isl_net_preprocess_crops. */
int isl_net_preprocess_crops_flip(isl_net* net, const uint8_t* d_frames, int n_frames, int H, int W,
                                  const isl_crop* crops, const uint8_t* flip, int n_crops,
                                  double scale_times_box, int* net_h, int* net_w, void* stream);

/* Run the network on the input buffer filled by isl_net_preprocess; outputs stay
 * in the arena (low-res, 8-channel chunks) for the post kernels, and are also
 * copied to d_out0/d_out1 (NCHW) when those are non-NULL. */
int isl_net_run(isl_net* net, float* d_out0, float* d_out1, void* stream);

/* Activation arenas (not in the reference: torch's caching allocator plays this
 * role there).  A net keeps one arena per net input size (h, w), sized by
 * capacity: a batch of n frames reuses an arena holding n' >= n frames, and a
 * larger n replaces it.  Arenas of other sizes are evicted least-recently-used
 * (ISL_ACT_FP16 runs keep arenas of their own per size, counted here like the others)
 * once the net's arenas would exceed the byte budget (env ISLPOSE_ARENA_BUDGET_MB,
 * default 65536; the arena in use is never evicted).  Reports the bytes held and
 * the number of arenas. */
int isl_net_arena_info(const isl_net* net, int64_t* bytes, int* n_arenas);

/* Select the conv arithmetic of a net (default ISL_ALGO_X3, or the env
 * ISLPOSE_CONV_ALGO=x3|wino|direct at create time). */
int isl_net_set_algo(isl_net* net, int algo);
int isl_net_get_algo(const isl_net* net);

/* Select the precision of a net's ISL_ALGO_X3 convs (default ISL_PREC_FP32, or the env
 * ISLPOSE_PRECISION=fp32|fp16 at create time); any other value -> ISL_E_ARG.  The hi-only
 * filters of ISL_PREC_FP16 are packed on the first run that needs them after a weight
 * upload and kept, so switching back and forth repacks nothing.  The range guard is
 * unchanged: an fp16-mode epilogue still flags |v| >= 65504, isl_net_check* still reports
 * ISL_E_RANGE, and the caller recomputes with ISL_ALGO_DIRECT.  Captured graphs
 * (isl_net_set_graph) are keyed by the precision.  isl_net_timing keeps kind 3 for these
 * launches and reports the FLOPs they execute (one product per multiply-add). */
int isl_net_set_precision(isl_net* net, int precision);
int isl_net_get_precision(const isl_net* net);

/* Select the activation storage of a net (default ISL_ACT_FP32, or the env
 * ISLPOSE_ACT_STORAGE=fp32|fp16 at create time); any other value -> ISL_E_ARG.  Arenas are
 * kept per (net size, storage), so switching back and forth reallocates nothing, and captured
 * graphs are keyed by the storage.  The range guard is unchanged: an epilogue checks the fp32
 * value before it rounds it, and the ISL_ALGO_DIRECT recompute runs on an fp32 arena.
 * isl_net_act_storage_active: 1 if the last run (or, before it, the last isl_net_preprocess*)
 * used fp16 activation buffers, else 0. */
int isl_net_set_act_storage(isl_net* net, int storage);
int isl_net_get_act_storage(const isl_net* net);
int isl_net_act_storage_active(const isl_net* net);

/* K ranges of the ISL_ALGO_X3 convolutions (latency of small grids such as batch-1
 * frames; not in the reference, whose torch conv runs per frame):
 *   mode 1 (default)  canonical ranges: layers of <= 1024 pixels per frame (Mode R's
 *                     23x41 body stages, the 184 px hand scale) sum their input
 *                     channels in up to 8 ranges fixed by the layer shape; a small grid
 *                     spreads the ranges over blocks (split-K, fixed-order reduction),
 *                     a large one keeps them in one block -- the same bits either way,
 *                     so a frame's maps do not depend on the batch it came in;
 *   mode 0            no ranges;
 *   mode 2            latency: mode 1, plus an adaptive split of every other layer
 *                     whose grid cannot half-fill the GPU (those layers' bits then
 *                     depend on the batch size, within the fp32 tolerance).
 * Env ISLPOSE_X3_SPLITK=0|1|2 sets the mode at create time. */
int isl_net_set_split_k(isl_net* net, int mode);

/* Graph replay of the conv chain (not in the reference: it replaces the per-op launches of
 * its torch module, src/model.py:171-207, with one HIP graph launch).  on = 1:
 * the first isl_net_run / isl_net_forward of a run key (batch size, K-range mode, conv
 * algorithm, ISLPOSE_* environment) on an arena runs eagerly, the second captures the
 * launches on a private stream and launches the graph on the caller's stream, later runs
 * replay it -- the same kernels with the same arguments, the same bits.  Timed runs
 * (isl_net_set_timing) stay eager; weight uploads and workspace growth drop the graphs.
 * on = 0 (default; replay measured level at batch 32 and slower at batch 1): every run
 * eager.  Env ISLPOSE_NET_GRAPH=0|1 turns replay off / on process-wide. */
int isl_net_set_graph(isl_net* net, int on);

/* A non-blocking stream for one lane of a pyramid's scales (not in the reference: its scales
 * run one after another on torch's current stream, body.py:47-77 / hand.py:31-50), created
 * with a priority class: -1 the device's greatest priority, 0 the middle of its range, +1 its
 * least.  HIP gives a process a few hardware queues per priority (GPU_MAX_HW_QUEUES, 4 by
 * default) and maps further streams onto them, so two scales on two streams of one priority
 * may still run one after the other; lanes of different priorities never share a queue, and
 * the command processor dispatches the high-priority lane (the largest scale, the critical
 * path) first.  *stream receives a hipStream_t; isl_lane_stream_destroy waits for its work
 * and frees it. */
int isl_lane_stream_create(int device, int priority_class, void** stream);
int isl_lane_stream_destroy(void* stream);

/* Range guard of ISL_ALGO_X3: waits for the device, returns ISL_E_RANGE if any
 * conv output since the last clear left the fp16 split range (the results of
 * those runs are then not fp32-accurate and must be recomputed with
 * ISL_ALGO_DIRECT), else ISL_OK; clear != 0 resets the flag.  The post records
 * of isl_body_post carry the same flag in their status word without a sync.
 * The flag also rises where nothing stored left the range but an intermediate did: a Winograd
 * input transform (up to 4 x the activations) that overflows the split, whatever the activation
 * then stores, and an isl_net_forward input outside the range. */
int isl_net_check(isl_net* net, int clear);
/* The same check stream-ordered, for pipelined callers: enqueues on `stream` a copy of
 * the flag into *h_flag (pinned host memory; valid once the stream has reached it) and
 * its reset.  *h_flag != 0 then means ISL_E_RANGE for the work enqueued before. */
int isl_net_check_async(isl_net* net, int32_t* h_flag, void* stream);
/* Range-guard diagnostics: *trips = how many checks (isl_net_check with clear != 0, and
 * isl_net_check_async once the stream has reached them) found the flag set, i.e. how
 * many batches the caller had to recompute on the fp32 kernels.  Waits for the device. */
int isl_net_range_info(isl_net* net, int64_t* trips);

/* Per-op device timing (measurement; not in the reference).  After
 * isl_net_set_timing(net, 1) every isl_net_run records a HIP event on its stream
 * before the first op and after each op.  isl_net_timing waits for the recorded
 * runs and returns, per op and summed over them: the duration in ms, the kind
 * (0 max-pool, 1 direct fp32 conv, 2 Winograd conv, 3 split-fp16 conv), the algorithmic FLOPs
 * (2*Cout*Cin*k*k*H*W*n, the direct-convolution count of SURVEY §8d) and the
 * FLOPs the matrix cores executed (tile padding included); then it drops the
 * events.  With op_ms == NULL it only reports *n_ops and *n_runs. */
int isl_net_set_timing(isl_net* net, int on);
int isl_net_timing(isl_net* net, int max_ops, int* n_ops, int* n_runs, double* op_ms, int* op_kind,
                   double* op_flops, double* op_mfma_flops);

/* Diagnostic: the ops of the net's graph (convs by their caffe layer name, pools as
 * "maxpool2") and, for the last isl_net_run / isl_net_forward, which conv kernel variant
 * each ran: for ISL_ALGO_X3 convs the variant code of csrc/internal.h x3_variant_code
 * (VAR bits: 1 reads or writes fp16 activations (ISL_ACT_FP16), 2 one-term fp16 products (ISL_PREC_FP16), 512 row union, 1024 in-block K ranges, 2048 split-K, 4096 two pairs per
 * step, 8192 folds its producers' split-K partials, 32768 pooled-input staging, 65536 one
 * input buffer, 131072 16x16x32 row union, 262144 conv1_1 kernel, 524288 split-K partials
 * left to its consumers (no reduce launch);
 * tile pixels / 32 at bits 20-24, output channels / 32 at bits 25-28, ks / 2 at 29-30);
 * -1 for a pool folded into the next conv's staging; 0 otherwise.  index < the op
 * count (isl_net_timing's *n_ops). */
int isl_net_op_info(const isl_net* net, int index, const char** name, int* variant);

/* Diagnostic: copy the net input buffer (filled by isl_net_preprocess) out as
 * float32 NCHW [n,3,net_h,net_w]. */
int isl_net_debug_input(isl_net* net, float* d_x_nchw, void* stream);

/* Capacities of the per-frame result records. */
typedef struct {
  int32_t max_peaks;   /* per part                                            */
  int32_t max_pairs;   /* candidate (i,j) pairs scored per limb (>= nA*nB)    */
  int32_t max_conns;   /* accepted connections per limb                       */
  int32_t max_rows;    /* subset rows during assembly                         */
} isl_caps;

/* Byte offsets inside one frame's result record (device memory, 8-byte aligned):
 *   int32  status                       ISL_OK / ISL_E_CAPACITY / ISL_E_INDEX
 *   int32  n_peaks[32]                  per part (body: njoint-1 parts)
 *   int32  n_conns[32]                  per limb, -1 = limb skipped (special_k)
 *   int32  n_rows                       subset rows after pruning
 *   double peaks[parts][max_peaks][3]   (x, y, score); id = running count
 *   double conns[limbs][max_conns][5]   (idA, idB, score, i, j)   body.py:171
 *   double subset[max_rows][njoint+1]                             body.py:182-231
 */
typedef struct {
  int64_t status, n_peaks, n_conns, n_rows, peaks, conns, subset, record_bytes;
} isl_layout;

int isl_body_layout(int model_kind, const isl_caps* caps, isl_layout* out);

/* Geometry of one scale of the pyramid (body.py:51-78): the net ran on a padded
 * input of net_h x net_w whose valid (un-padded) part is valid_h x valid_w. */
typedef struct {
  int32_t net_h, net_w;       /* padded net input size (multiples of 8)         */
  int32_t valid_h, valid_w;   /* resized image size before padding              */
} isl_scale_geom;

/* Body post-processing (body.py:64-235) for n frames of size H x W.
 * For each scale s, low-res maps are read from d_paf[s] / d_heat[s] (float32
 * NCHW [n,C,net_h/8,net_w/8]); NULL entries mean "use the net's own arena
 * output" (valid only for nscales == 1, right after isl_net_run).
 * Results: n records of isl_body_layout(...).record_bytes at d_result. */
int isl_body_post(isl_net* net, int n, int H, int W, int nscales, const isl_scale_geom* geom,
                  const float* const* d_paf, const float* const* d_heat,
                  const isl_caps* caps, void* d_result, void* stream);

/* Hand post-processing (hand.py:51-74) for n crops of size h x w: per scale,
 * low-res hand maps (NCHW [n,22,net_h/8,net_w/8], NULL = the net's arena output
 * for nscales == 1) -> int64 peaks [n][21][2] as (x, y), [0, 0] when no pixel of
 * the blurred part map exceeds 0.05. */
int isl_hand_post(isl_net* net, int n, int h, int w, int nscales, const isl_scale_geom* geom,
                  const float* const* d_heat, int64_t* d_peaks, void* stream);

/* Run-time options of the post-processing (constants in the reference):
 *   thre1       body peak threshold: a pixel is a peak only if the blurred map there
 *               is > thre1 (body.py:43, used at :99-100); default 0.1
 *   thre2       PAF sample threshold: a pair passes when more than 0.8 * mid_num of its
 *               samples are > thre2 (body.py:44, used at :157-160); default 0.05
 *   hand_thre   hand map threshold: binary = blurred > hand_thre (hand.py:62); default 0.05
 *   max_people  not in the reference; 0 = no cap (default).  After the pruning of
 *               body.py:227-231, when more than max_people subset rows remain, the
 *               max_people rows with the largest total score (subset[:, -2]) are kept,
 *               ties going to the lower row, in their original order.  candidate is
 *               unchanged and ISL_E_INDEX (body.py:196) is raised as without a cap.
 * Accepted: thre1 and hand_thre finite in [1e-30, 1e30] (an all-zero map must have an
 * all-zero mask, and the fp32 blur filter's margins are relative to the threshold: they
 * hold while it is a normal fp32 number), thre2 finite, max_people >= 0, reserved zero;
 * anything else is ISL_E_ARG.  isl_post_opts_default fills in the defaults. */
typedef struct {
  double thre1, thre2, hand_thre;
  int32_t max_people;
  int32_t reserved[3];
} isl_post_opts;

int isl_post_opts_default(isl_post_opts* opts);

/* isl_body_post (body.py:64-235) with thre1 (body.py:43), thre2 (body.py:44) and
 * max_people of `opts`; NULL: the defaults, which is isl_body_post. */
int isl_body_post_opts(isl_net* net, int n, int H, int W, int nscales, const isl_scale_geom* geom,
                       const float* const* d_paf, const float* const* d_heat,
                       const isl_caps* caps, void* d_result, void* stream, const isl_post_opts* opts);

/* isl_hand_post (hand.py:51-74) with hand_thre of `opts` for hand.py:62's 0.05; NULL: the
 * defaults, which is isl_hand_post. */
int isl_hand_post_opts(isl_net* net, int n, int h, int w, int nscales, const isl_scale_geom* geom,
                       const float* const* d_heat, int64_t* d_peaks, void* stream,
                       const isl_post_opts* opts);

/* Hand post-processing of n square crops of different sizes in one call
 * (HandEstimator.post_crops; hand.py:51-74 per crop): crop i is crop_w[i] px (host
 * array), geom[i*nscales + si] its geometry at scale si (host), its low-res maps crop
 * i of d_heat[si] (NCHW [n,22,net_h/8,net_w/8]; every crop has the same net size per
 * scale) -> int64 peaks [n][21][2].  Stream-ordered on `stream`: the crops run side by
 * side on the net's internal post streams, forked from and joined back into it.  The
 * batch's stage-1 maps live in a buffer of their own whose next writer waits (on the
 * device) for the lanes of the previous call, whatever stream either runs on.
 * Host synchronisation: only when a call needs more lane or stage-1 scratch than any
 * call before it does it wait for that buffer's earlier readers before reallocating
 * (once per new maximum size); otherwise it never blocks the host. */
int isl_hand_post_crops(isl_net* net, int n, const int32_t* crop_w, int nscales,
                        const isl_scale_geom* geom, const float* const* d_heat, int64_t* d_peaks,
                        void* stream);

/* isl_hand_post_crops with hand_thre of `opts` for hand.py:62's 0.05 in every crop's post;
 * NULL: the defaults, which is isl_hand_post_crops. */
int isl_hand_post_crops_opts(isl_net* net, int n, const int32_t* crop_w, int nscales,
                             const isl_scale_geom* geom, const float* const* d_heat, int64_t* d_peaks,
                             void* stream, const isl_post_opts* opts);

/* isl_hand_post_opts / isl_hand_post_crops_opts with two more arguments (not in the reference):
 *   flip      host array, one flag per crop, NULL for none: crop i's maps are those of the
 *             mirrored crop (isl_net_preprocess_crops_flip).  The whole post runs unchanged in
 *             the coordinates of the image the net saw; only the final store mirrors the x of
 *             a detected part back into the caller's crop: x -> w - 1 - x.
 *   d_scores  device double [n][21], NULL for not wanted: for a part whose thresholded map is
 *             not empty (np.sum(binary) != 0, hand.py:63) the value of map_ori at the returned
 *             pixel after hand.py:70's masking -- the scale-averaged map there, which OpenPose
 *             reports as the keypoint's confidence; for an empty part 0.0.
 * An empty part stays [0, 0] with score 0.0, mirrored or not, so a score > 0 tells "found at
 * the origin" from "nothing found".  Both NULL: the _opts entry points. */
int isl_hand_post_ex(isl_net* net, int n, int h, int w, int nscales, const isl_scale_geom* geom,
                     const float* const* d_heat, int64_t* d_peaks, void* stream,
                     const isl_post_opts* opts, const uint8_t* flip, double* d_scores);
int isl_hand_post_crops_ex(isl_net* net, int n, const int32_t* crop_w, int nscales,
                           const isl_scale_geom* geom, const float* const* d_heat, int64_t* d_peaks,
                           void* stream, const isl_post_opts* opts, const uint8_t* flip,
                           double* d_scores);

/* Diagnostic: numpy's np.sum of a float64 array (pairwise 8192-element buffers added
 * left to right, hand.py:68's association) as the hand post computes it for component
 * sums (the block-cooperative device routine): d_out[0] = sum(d_a[0..n)). */
int isl_debug_np_sum(const double* d_a, int64_t n, double* d_out, void* stream);

/* Diagnostic: the host-side choices of the post-processing, as data -- which kernel forms and
 * which blur branch isl_body_post_opts / isl_hand_post* take for a geometry and the A/B
 * environment switches as they stand at the call.  The posts call the same two host functions
 * and launch from their result, so a test that asserts a plan asserts the branch a post at that
 * geometry reaches.  Neither entry touches the device or needs a net.
 *
 * One launch of the separable resize (resize_sep_kernel): */
typedef struct {
  int32_t launched;   /* 0: the post launches no such resize (the fields below are zero)        */
  int32_t ty;         /* output rows per tile (64 unless the source window caps it)             */
  int32_t cols;       /* output columns per block: 128 or 256                                   */
  int32_t v4;         /* the four-column vertical pass (needs width % 4 == 0, ty % 4 == 0)      */
  int32_t bm;         /* also writes the band maxima of its output (needs ty % 16 == 0)         */
  int32_t identity;   /* the source is copied, not interpolated                                 */
} isl_resize_plan;

enum isl_blur_branch {
  ISL_BLUR_MULTI_F64 = 0,    /* several scales: fp64 average planes, one block per tile          */
  ISL_BLUR_FUSED_LIVE = 1,   /* resize inside the blur, over the live-tile list                  */
  ISL_BLUR_BAND_LIVE = 2,    /* materialised fp32 planes, live-tile list from the band maxima    */
  ISL_BLUR_DENSE = 3         /* materialised fp32 planes, one block per tile of the dense grid   */
};

#define ISL_PLAN_SCALES 8    /* the posts take at most this many scales */

typedef struct {
  int32_t multi;        /* nscales > 1                                                          */
  int32_t two_stage;    /* single scale whose valid size is not the frame's (x8, then to frame) */
  int32_t fused;        /* no full-resolution heat planes: the blur resizes on the fly          */
  int32_t fuse2;        /* two_stage and fused (the stage-2 window fits the blur's LDS window)  */
  int32_t wide;         /* fuse2 through the wide window (development build only)               */
  int32_t skip2;        /* stage-2 tiles no live blur window reads are skipped                  */
  int32_t blur;         /* enum isl_blur_branch                                                 */
  int32_t blur_bandmax; /* ISL_BLUR_DENSE only: the tiles still take the band-maxima early out  */
  int32_t acc_ty;       /* multi: resize_acc_kernel's output rows per tile (16 or less); else 0 */
  int32_t stage2_ty;    /* output rows per stage-2 resize tile as stage2_need_kernel counts them */
  int32_t limb_z;       /* blocks per limb of the pair scoring (1: the one-kernel form)         */
  /* the environment switches as read: 1 = on */
  int32_t env_fused_blur, env_fused_wide, env_blur_list, env_blur_bands, env_resize_skip, env_resize_v4;
  int32_t env_blur_exact;   /* ISLPOSE_BLUR_EXACT: 0, 1 or 2                                    */
  int32_t scale_two_stage[ISL_PLAN_SCALES];   /* per scale: valid size != frame size            */
  isl_resize_plan stage1[ISL_PLAN_SCALES];    /* x8 to the valid size (two-stage scales only)   */
  isl_resize_plan final_rs[ISL_PLAN_SCALES];  /* the resize that lands on the frame; launched   */
                                              /* only for a single scale that is not fused      */
  int32_t env_limb_lds;     /* ISLPOSE_LIMB_LDS: large pair sets ranked and matched in LDS      */
  int32_t env_asm_reg;      /* ISLPOSE_ASM_REG: the assembly's merge in registers               */
  int32_t reserved[4];
} isl_body_post_plan;

typedef struct {
  int32_t two_stage[ISL_PLAN_SCALES];   /* per scale: valid size != crop size                   */
  int32_t identity[ISL_PLAN_SCALES];    /* per scale: the accumulate kernel copies the source   */
  isl_resize_plan stage1[ISL_PLAN_SCALES];   /* x8 to the valid size (two-stage scales only)    */
  int32_t acc_ty;       /* resize_acc_kernel's output rows per tile: 16, less when a scale's    */
                        /* source rows per output row would overflow the 40-row LDS window      */
  int32_t cc_lds;       /* 1: components in one workgroup's LDS (h * w <= 36864); 0: the        */
                        /* large-plane chain                                                    */
  int32_t cc_rows, cc_chunks;   /* the large-plane chain's rows per chunk and chunks per plane  */
  int32_t reserved[4];
} isl_hand_post_plan;

/* model_kind ISL_BODY25 / ISL_COCO, n frames of H x W, geom[nscales].  ISL_E_ARG: a NULL, a
 * non-positive size, nscales outside 1..ISL_PLAN_SCALES, a net size below 8 or a valid size
 * below 1. */
int isl_debug_body_post_plan(int model_kind, int n, int H, int W, int nscales, const isl_scale_geom* geom,
                             isl_body_post_plan* out);
int isl_debug_hand_post_plan(int h, int w, int nscales, const isl_scale_geom* geom, isl_hand_post_plan* out);

/* Diagnostic: one 3x3 convolution layer (stride 1, pad 1, bias, PReLU) of the split-fp16 path on
 * host arrays, outside any net -- shapes no graph has, such as a K loop of one or two steps.
 * x [n][cin][h][w], wgt [cout][cin][3][3], bias and slope [cout], y [n][cout][h][w], all fp32 on
 * the host; cin a multiple of 8.  kernel 0: conv_x3; 1: the Winograd kernel (wino_f16), ISL_E_ARG
 * when the shape is not eligible for it (cout % 64, >= 32 tiles per row, > 1024 pixels).  The call
 * is synchronous on the current device; ISL_E_RANGE when the layer left the fp16 split range. */
int isl_debug_conv3x3(const float* x, int n, int cin, int h, int w, const float* wgt, const float* bias,
                      const float* slope, int cout, int kernel, float* y);

/* Diagnostic: one convolution layer on any of the conv kernels, on host arrays, outside any net,
 * synchronous on the current device -- the per-layer entry of the test suite (tests/
 * test_gpu_conv_layers.py).  It builds the buffers a net would give the launch (rings, channel
 * slices, a channel map of segments), runs the launcher the descriptor names and reports, beside
 * the result, what the launch wrote outside its footprint.
 *
 *   x      [n][cin][h][w] fp32, logical channel order; with `vin` the pre-pool map [n][cin][2h][2w]
 *   wgt    [cout][cin][ks][ks], bias [cout], slope [cout] (PReLU only; NULL otherwise)
 *   y      [n][cout][h][w]; with `hpool` the pair-max map [n][cout][h][w/2]
 *   y_pool with `hpool`: [n][cout][h/2][w/2], the map launch_vpool2 makes of it (floor mode); else NULL
 *
 * Buffers.  The input buffer has in_cs physical channels in 8-channel chunks and a ring of in_pad
 * pixels; the layer reads channels [in_coff, in_coff + P), P = the segments' extent rounded up to 8.
 * Segment i puts logical channels [logical, logical + len) at physical offset phys inside that
 * span (the cmap of a concat buffer: 52 PAF channels in a 56-channel slot, then 128 features).
 * Rings and gap channels of the layer's own chunks are zero, as plan() leaves them; every other
 * chunk, and a slack (a chunk plane + 1024 pixels) on either side of the buffer, holds a NaN
 * (payload 0x51d1d1), so a
 * kernel that reads them shows it in its result.  The output buffer has out_cs channels and a ring
 * of out_pad; the layer writes (frame interior) x [out_coff, out_coff + cout).  Before the launch
 * the whole buffer and the same slack on either side hold a canary no layer can produce (the quiet
 * NaN 0x7fc5a5a5, fp16 0x7e5a); after it every element outside the footprint whose bits differ
 * counts as a stray write -- rings, channels [cout, round8(cout)), other slices, the slack.
 * With `act16` the input and output buffers hold fp16 (x rounded to nearest even by the entry; the
 * rgb kernel reads its fp32 input as ever); y is returned as fp32.  With `vin` the entry builds the
 * pool's pair-max buffer [n][chunk][2h][w][8] (max of horizontal pairs, exact) and the launch stages
 * from it.  With `hpool` the launch writes the unpadded pair-max buffer (checked as above); the
 * entry then zeroes that buffer's gap channels (the arena's one-time zeroing) and runs
 * launch_vpool2 into a canary-filled buffer of ring out_pad, whose footprint is whole chunks:
 * gap lanes there must read +0.
 *
 * ISL_E_ARG: a malformed descriptor, a shape the named kernel does not take (x3_fits,
 * wino_f16_fits, x3_rgb_fits, x3_hpool_ok, x3_vin_ok, x3_act16_ok, wino_bco_for), or a call over
 * the limits (n <= 256, h * w <= 2^20, channels <= 1024, each buffer <= 256 MiB).
 * ISL_E_RANGE only when range_error != 0 and the layer raised the range flag.
 *
 * Not reachable here: the fused conv1_1 -> conv1_2 launch, the fused 1x1 pair and the split-K
 * fold.  The suite holds them bit for bit to their unfused forms at net level
 * (tests/test_gpu_fused.py, tests/test_gpu_fp16_fused.py); the unfused forms are checked here. */
enum isl_debug_kernel {
  ISL_DBG_X3 = 0,      /* launch_conv_x3: the dispatcher picks the variant          */
  ISL_DBG_WINO2 = 1,   /* launch_wino_f16                                           */
  ISL_DBG_DIRECT = 2,  /* launch_conv (fp32 matrix cores; the range guard's fallback) */
  ISL_DBG_WINO = 3,    /* launch_wino (fp32 Winograd)                               */
  ISL_DBG_RGB = 4      /* launch_conv_x3_rgb (cin = 3)                              */
};

typedef struct {
  int32_t phys, logical, len;
} isl_debug_seg;

typedef struct {
  int32_t n, h, w;                 /* frames; the plane the convolution runs on               */
  int32_t cin, cout;               /* logical channels                                        */
  int32_t ks;                      /* 1, 3, 7                                                 */
  int32_t act;                     /* 0 none, 1 ReLU, 2 PReLU                                 */
  int32_t kernel;                  /* enum isl_debug_kernel                                   */
  int32_t f16;                     /* one-term products (ConvLaunch::f16, hi-only filters)    */
  int32_t act16;                   /* fp16 buffers (ConvLaunch::act16); needs f16             */
  int32_t allow_split;             /* 0 / 1: canonical K ranges, with a split-K workspace     */
  int32_t in_pad, out_pad;         /* rings: 1 or 3, in_pad >= ks / 2                         */
  int32_t in_cs, in_coff;          /* input buffer channels, the layer's offset (multiples of 8) */
  int32_t out_cs, out_coff;        /* output buffer channels, the layer's offset              */
  int32_t nseg;                    /* 1..4                                                    */
  isl_debug_seg seg[4];
  int32_t hpool, vin;              /* conv_x3 only                                            */
  int32_t range_error;             /* != 0: a raised range flag returns ISL_E_RANGE           */
  int32_t reserved[7];             /* zero                                                    */
} isl_debug_conv_desc;

typedef struct {
  int32_t variant;       /* the launch's variant code (x3, rgb); for wino2 the code the runtime gives  */
                         /* launch_wino_f16 (a constant: that launcher has no variants and is  */
                         /* called directly); 0 for direct / wino                              */
  int32_t range_flag;    /* the launch's range flag as a value                                */
  int64_t stray_writes;  /* elements outside the footprint whose bits changed                 */
  int64_t unwritten;     /* footprint elements still holding the canary                       */
  int32_t stray_stage;   /* the first stray write: 0 the conv's output buffer, 1 the pooled   */
  int32_t stray_frame;   /*   map; frame -1 = the slack before (chunk -1) or after (chunk 1)  */
  int32_t stray_chunk;   /*   the buffer, x then counting elements; y, x relative to the      */
  int32_t stray_y;       /*   frame interior (negative or >= the size: the ring)              */
  int32_t stray_x;
  int32_t stray_lane;
  int32_t reserved[6];
} isl_debug_conv_result;

int isl_debug_conv(const isl_debug_conv_desc* desc, const float* x, const float* wgt, const float* bias,
                   const float* slope, float* y, float* y_pool, isl_debug_conv_result* result);

/* Sign classifier of ISLSignPosTranslator (reference demo_isl_translate.py:72-100,
 * applied in src/ISL_Model_parameter.py:337 to a [1,20,156] window of
 * populate_features rows, :376-443): Masking(0) -> BatchNorm -> BiLSTM(32, seq)
 * -> BiLSTM(32) -> elu -> Dense32 -> BN -> elu -> Dense32 -> BN -> elu ->
 * Dense(n_classes) softmax, inference semantics (dropouts off, keras masking).
 * d_params: float32, the keras `model.get_weights()` list flattened in order
 * (isl_sign_param_count floats); d_windows: float32 [batch][window][n_features];
 * d_probs: float32 [batch][n_classes].  window <= 32, n_features <= 256,
 * n_classes <= 1024.  One workgroup per window, one launch per call. */
int isl_sign_param_count(int n_features, int n_classes, int64_t* count);
int isl_sign_classify(const float* d_params, int n_features, int window, int n_classes,
                      const float* d_windows, int batch, float* d_probs, void* stream);

/* Training step of the sign classifier: the per-window loss and the gradient of the batch loss
 * with respect to every parameter, forward and backward through time in one launch (one
 * workgroup per window) plus one reduction launch.  DESIGN.md section 4.2k holds the definition.
 *   model     the stack of isl_sign_classify with the same parameter layout; the three batch
 *             normalisations use their stored moving statistics (frozen), so the gradient entries
 *             of the 2 * n_features + 4 * 32 mean and variance slots are written as 0.
 *   loss      l_b = logsumexp(logits_b) - logits_b[label_b]; L = (1 / batch) * sum_b w_b * l_b.
 *             A label outside [0, n_classes) ignores the window: l_b = 0, no gradient, still
 *             counted in batch.  d_weights NULL: every w_b is 1.
 *   dropout   opts NULL: none.  Otherwise rates p_drop (the three Dropout layers) and p_rec (the
 *             recurrent dropout of the four LSTM directions, one mask per direction and window
 *             held over all steps), each in [0, 0.9], 0 = the site is off.  Draws are
 *             counter-based: k = sm(sm(sm(seed ^ step) ^ id_b) ^ (site << 32 | index)) with the
 *             splitmix64 finaliser sm; an element is kept iff (k >> 40) >= floor(rate * 2^24 + 0.5)
 *             and a kept value is multiplied by the fp32 1.0f / (1.0f - rate).  d_ids NULL:
 *             id_b = b.  A window's masks depend on neither its batch nor its place in it.
 *   d_loss    float32 [batch], l_b.        d_grad    float32 [isl_sign_param_count], dL/dtheta.
 *   d_workspace   isl_sign_grad_workspace bytes: one gradient slice per
 *             workgroup (min(batch, 256) of them); workgroup j adds windows j, j + G, ... in that
 *             order into its slice and the second launch adds the slices in index order.  No
 *             float atomics: the same inputs give the same bits, and l_b does not depend on the
 *             batch.
 * ISL_E_ARG, before any device work, for: a NULL d_params, d_windows, d_labels, d_loss or
 * d_workspace with batch > 0, a NULL d_grad, batch < 0, window outside [1, 32], n_features outside
 * [1, 256], n_classes outside [1, 1024], a rate that is not a number in [0, 0.9], reserved not
 * zero.  batch == 0 writes a zero gradient and returns. */
typedef struct {
  float p_drop, p_rec;
  uint64_t seed, step;
  int32_t reserved[4];
} isl_sign_train_opts;

int isl_sign_train_opts_default(isl_sign_train_opts* opts);   /* 0.2, 0.2, seed 0, step 0 */
int isl_sign_grad_workspace(int n_features, int n_classes, int batch, int64_t* bytes);
int isl_sign_grad(const float* d_params, int n_features, int window, int n_classes,
                  const float* d_windows, const int32_t* d_labels, const float* d_weights,
                  const uint64_t* d_ids, int batch, const isl_sign_train_opts* opts, float* d_loss,
                  float* d_grad, void* d_workspace, void* stream);

/* Keypoint-space augmentation of the classifier's windows, in one launch (csrc/sign_augment.hip;
 * DESIGN.md section 4.2m holds the definition).  Output window k, float32 [window][n_features], is
 * item k's view of a resident row store d_rows [n_rows][n_features]:
 *   rows      n_features = 2 * n_body + n_slots * 3 * n_hand: n_body x, n_body y, then per hand slot
 *             n_hand x, n_hand y, n_hand labels.  A pair (x, y) is absent iff both values are 0.
 *   frames    output frame t reads source row
 *             r = floor(((2t - (window-1)) * q + 16 * (window-1) + 16) / 32) + start of the item's
 *             source d_rows[row0 .. row0 + nrows); r outside [0, nrows) gives an all-zero frame, and
 *             so does a dropped frame: (sm(kw ^ (16 << 32 | t)) >> 40) < floor(drop * 2^24 + 0.5),
 *             kw = sm(sm(seed ^ step) ^ id), sm the splitmix64 finaliser of isl_sign_grad.
 *   pairs     of a live frame, in fp64 without fused multiply-adds: X = (m0*x + m1*y) + m2,
 *             Y = (m3*x + m4*y) + m5; with jitter > 0, X += jitter * (u * 2^-23 - 1) with
 *             u = sm(kw ^ (17 << 32 | (t * 512 + 2p))) >> 40, p the pair's index in the row, and Y
 *             the same with index + 1; both rounded once to fp32; if both are then 0, x is stored as
 *             2^-10 (a present point never turns absent).  Absent pairs are stored as (0, 0); labels
 *             are copied.  Points are not clipped to any frame.
 *   items     an item with nrows < 1, q outside [8, 32], row0 < 0 or row0 + nrows > n_rows gives an
 *             all-zero window; no row outside the store is addressed.
 * A window depends only on its item, the rows it names and (seed, step, drop, jitter).  d_windows
 * must not overlap d_rows.  Plain loads and stores, no host synchronisation.
 * ISL_E_ARG, before any device work, for: n_items < 0 or > 65535, and with n_items > 0 a NULL
 * pointer, n_rows < 0, window outside [1, 32], n_features outside [1, 256], a negative layout count,
 * a layout whose size is not n_features, drop not a number in [0, 0.9], jitter not finite and >= 0,
 * a reserved field not zero.  n_items == 0 returns at once. */
typedef struct {
  int64_t row0;      /* first row of the source (a clip, or a pre-cut window) in d_rows */
  int32_t nrows;     /* rows of the source, >= 1 */
  int32_t start;     /* source row of output frame 0 at speed 1; may be negative */
  int32_t q;         /* speed in 1/16: 16 = as recorded; in [8, 32] */
  int32_t reserved;  /* 0 */
  uint64_t id;       /* sample id of the draws made in the kernel */
  double m[6];       /* x' = (m0*x + m1*y) + m2;  y' = (m3*x + m4*y) + m5 */
} isl_sign_aug_item; /* 80 bytes */

typedef struct {
  int32_t n_body, n_slots, n_hand, reserved;
} isl_sign_aug_layout;

typedef struct {
  float drop, jitter;
  uint64_t seed, step;
  int32_t reserved[4];
} isl_sign_aug_opts;

int isl_sign_aug_opts_default(isl_sign_aug_opts* opts);   /* 0, 0, seed 0, step 0 */
int isl_sign_augment(const float* d_rows, int64_t n_rows, int n_features, const isl_sign_aug_layout* layout,
                     const isl_sign_aug_item* d_items, int n_items, int window,
                     const isl_sign_aug_opts* opts, float* d_windows, void* stream);

/* ---- augmented copies of resident frames --------------------------------- */

/* One variant of a uint8 [H,W,3] frame, the reference's dataset augmentation
 * (extract_featuressingle.py:49-52,116-120: v2.RandomRotation, v2.RandomSolarize, torchvision
 * v2's tensor path; that parity is unpinned, the library being absent -- DESIGN.md section 4.2h
 * holds the definition): the rotation first, then the solarize; either may be off.
 *   rotation   by `angle` degrees, counter-clockwise for positive angles, about the image centre,
 *              nearest neighbour, same size, fill 0.  The caller passes c = cos(r), s = sin(r) of
 *              r = radians(-angle), so no device libm enters.  In fp64, in this order, without
 *              fused multiply-adds: cx = (W-1)*0.5, cy = (H-1)*0.5; for output pixel (row j,
 *              column i) dx = i - cx, dy = j - cy, xs = (c*dx + s*dy) + cx,
 *              ys = ((-s)*dx + c*dy) + cy, xi = rint(xs), yi = rint(ys) (half to even); the
 *              pixel is src[yi, xi, :] where 0 <= xi < W and 0 <= yi < H, else 0.
 *   solarize   a byte v becomes 255 - v where v >= threshold; threshold in [0, 256], 256 = off.
 *              Filled pixels go through it too.
 *   swap_rb    output channel k is source channel 2 - k (applied at the load, so it commutes
 *              with both transforms): the RGB -> BGR flip of extract_features_mp.py:124.
 * An item with everything off is a plain copy of frame `src`. */
typedef struct {
  double c, s;          /* cos / sin of radians(-angle); read only when rotate != 0 (finite) */
  int32_t src;          /* source frame index in [0, n_src)                                  */
  int32_t rotate;       /* 0 / 1                                                             */
  int32_t threshold;    /* solarize threshold in [0, 256]; 256 = off                         */
  int32_t swap_rb;      /* 0 / 1                                                             */
  int32_t reserved[2];  /* zero                                                              */
} isl_aug_item;

/* dst[k] = variant(src[items[k].src], items[k]) for k < m, in one launch on `stream`:
 * d_src uint8 [n_src,H,W,3], d_dst uint8 [m,H,W,3], both on the current device; `items` is a
 * host array of m records, uploaded stream-ordered through a pinned ring (the call does not
 * wait for the stream unless eight earlier calls are still in flight).  m == 0 is a no-op.
 * ISL_E_ARG, before any device work, for: a NULL buffer, n_src, H or W <= 0, H*W > 2^29, m < 0
 * or m > 65535, a src index outside [0, n_src), a threshold outside [0, 256], rotate or swap_rb
 * not 0 / 1, a non-finite c or s of a rotating item, a non-zero reserved field, or d_dst
 * overlapping d_src. */
int isl_augment(const uint8_t* d_src, int n_src, int H, int W, uint8_t* d_dst,
                const isl_aug_item* items, int m, void* stream);

/* ---- stick-model overlays on resident frames ------------------------------ */

/* One drawing primitive of the stick-model picture the reference writes beside each keypoint
 * JSON (util.drawStickmodel / draw_bodypose / draw_handpose, src/util.py:47-96,154-185,308-358;
 * extract_features_mp.py:85-91).  Parity with cv2's polygon rasteriser and matplotlib's
 * antialiased lines is unpinned (both are absent); DESIGN.md section 4.2j holds this exact integer
 * definition, which the kernel, islpose.render.apply_numpy and the tests share byte for byte.
 *
 * A frame is uint8 [H,W,3]; `color` goes to channels 0, 1, 2 as given (the caller orders it for
 * RGB or BGR).  A frame's primitives are applied in list order: the blend does not commute.  All
 * arithmetic is in 64-bit integers; (x, y) is the pixel (column, row), dx = x - cx, dy = y - cy.
 *   kind 0  stick    p = cx, cy, a, b: half axes a in [1, 4096], b in [1, 16]; c, s =
 *                    round(cos(t) * 16384), round(sin(t) * 16384) of the angle t, computed by the
 *                    caller.  u = dx*c + dy*s, v = -dx*s + dy*c; covered iff |u| <= a*2^14 and
 *                    |v| <= b*2^14 and u^2*b^2 + v^2*a^2 <= a^2*b^2*2^28 (the first two tests
 *                    come first: they keep the squares under 2^63).
 *   kind 1  disc     p = cx, cy; covered iff dx^2 + dy^2 <= r2, r2 in [0, 4096].
 *   kind 2  segment  p = x0, y0, x1, y1, r2 in [0, 4096]: with d = P1 - P0, L2 = d.d,
 *                    w = (x, y) - P0, t = w.d, cr = w.x*d.y - w.y*d.x, covered iff
 *                    (L2 > 0 and 0 <= t <= L2 and cr^2 <= r2*L2) or |w|^2 <= r2 or
 *                    |(x, y) - P1|^2 <= r2.  L2 = 0 is the disc: t and cr are 0 at every pixel
 *                    then, so the first test is taken only for L2 > 0.
 *   colouring        a covered channel value v under colour k becomes k (blend 0) or
 *                    (4*v + 6*k + 5) / 10 rounded down (blend 1), which is rint(0.4*v + 0.6*k)
 *                    for all 65536 pairs: what cv2.addWeighted(canvas, 0.4, cur, 0.6, 0) leaves
 *                    inside a limb, while outside it leaves v.
 * Limits: every coordinate (cx, cy, x0, y0, x1, y1) in [-16384, 16384], |c|, |s| <= 16384,
 * H, W <= 16384, H*W <= 2^29.  Parts of a primitive off the frame are clipped.  Fields a kind
 * does not use (a disc's p[2], p[3], c, s; a segment's c, s; a stick's r2) are not read. */
typedef struct {
  int32_t kind, p[4], c, s, r2;
  uint8_t color[3], blend;
  int32_t reserved;   /* zero */
} isl_draw_prim;

/* Draws frame f's primitives prims[first[f] .. first[f+1]) onto frame f, for f < n, in one launch
 * on `stream`: d_src, d_dst uint8 [n,H,W,3] on the current device; `prims` and `first` (n + 1
 * entries) are host arrays, uploaded stream-ordered through a pinned ring (the call does not wait
 * for the stream unless eight earlier calls are still in flight).
 *   d_dst == d_src            in place; a pixel tile no primitive touches is never written
 *   d_dst disjoint from d_src dst = the copy of src with the drawing
 *   d_src == NULL             dst = the drawing on an all-zero canvas
 * n == 0, or no primitives in place: a no-op; no primitives otherwise: the plain copy (or zeros).
 * ISL_E_ARG, before any device work, for: a NULL d_dst, d_src and d_dst overlapping without being
 * equal, n < 0, H or W outside [1, 16384], H*W > 2^29, a NULL `first` (n > 0), first[0] != 0, a
 * decreasing `first`, more than 2^20 primitives, a NULL `prims` with primitives to draw, an
 * unknown kind, blend not 0 / 1, a parameter a kind reads outside the limits above, or a non-zero
 * reserved field. */
int isl_draw(const uint8_t* d_src, uint8_t* d_dst, int n, int H, int W,
             const isl_draw_prim* prims, const int32_t* first, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISLPOSE_H */
