/* yogo_hip.h -- C ABI of libyogo_hip.so, the MI355X (gfx950) implementation of the YOGO hot path.
 *
 * The reference (czbiohub-sf/yogo @ 2024_08_07) has no native code and no FFI: its "operators" are torch ATen /
 * cuDNN / torchvision calls made from Python.  Each entry point below names the reference call site it replaces
 * (file:line relative to the reference root).  How a maintainer binds them (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless noted; tensors are contiguous NCHW fp32 unless noted
 *   - nothing is allocated or freed here: the caller passes outputs and workspaces (sizes from *_bytes / *_rows)
 *   - hipStream_t is passed as an opaque pointer; all work is enqueued on it, no host synchronisation
 *   - return value 0 = ok; non-zero = error, message from yogo_hip_last_error() (thread-local)
 *   - re-entrant; one host thread per device
 *   - activation codes: 0 none, 1 LeakyReLU(0.01), 2 SiLU
 */
#ifndef YOGO_HIP_H
#define YOGO_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* yogo_stream_t; /* hipStream_t */

const char* yogo_hip_last_error(void);
int yogo_hip_abi_version(void);
/* Launch log (test / profiling aid, no counterpart in the reference): while enabled, every entry point that launches a
 * convolution / weight-gradient kernel appends one line "<kernel instantiation as rocprofv3 names it> | <planner parameters>".
 * enable = 1 clears and starts recording, 0 stops.  yogo_hip_launch_log_read copies the text into a HOST buffer (NUL
 * terminated, truncated to cap) and reports the bytes needed. */
int yogo_hip_launch_log(int enable);
int yogo_hip_launch_log_read(char* buf, size_t cap, size_t* needed);

/* ---- convolution, fp32 matrix cores ---------------------------------------------------------------------------
 * nn.Conv2d(cin, cout, 3, stride=1|2, padding=1) and nn.Conv2d(cin, cout, 1): yogo/model_defns.py:34-67,
 * executed at yogo/model.py:275 (forward) and by loss.backward() at yogo/train.py:322 (dgrad / wgrad).          */

/* bytes of the packed weight buffer. mode 0: forward, mode 1: dgrad */
int yogo_conv_packed_bytes(int Cin, int Cout, int ksize, int stride, int mode, size_t* bytes);
/* OIHW weights -> packed [tap][Kpad][Mpad] */
int yogo_conv_pack_f32(const float* w_oihw, float* packed, int Cin, int Cout, int ksize, int stride, int mode,
                       yogo_stream_t stream);
/* rows / row stride (floats/2) of the BatchNorm partial-sum buffer a forward launch fills when stats_part != NULL */
int yogo_conv2d_fwd_stats_shape(int B, int Cin, int Cout, int IH, int IW, int ksize, int stride, int* rows, int* mpad);
/* out = chan_scale[b][c] * act(conv(in) + bias); out_pre (optional) receives conv(in)+bias;
 * stats_part (optional) receives per-workgroup (sum, sumsq) per channel for BatchNorm training statistics.
 * Fuses Conv2d + bias + LeakyReLU/SiLU + Dropout2d channel mask (model_defns.py:39-41 etc.).                      */
int yogo_conv2d_fwd_f32(const float* in, const float* packed, const float* bias, float* out, float* out_pre,
                        const float* chan_scale, float* stats_part, int B, int Cin, int Cout, int IH, int IW, int ksize,
                        int stride, int act, yogo_stream_t stream);
/* dx = conv_transpose(dy) * act'(act_ref) * chan_scale   (act_ref / chan_scale optional).
 * (IH, IW) are the forward conv's INPUT dims.  act_ref: block output for LeakyReLU, pre-activation for SiLU.      */
int yogo_conv2d_dgrad_f32(const float* dy, const float* packed_dgrad, float* dx, const float* act_ref, int ref_act,
                          const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ksize, int stride,
                          yogo_stream_t stream);
int yogo_conv2d_wgrad_workspace_bytes(int B, int Cin, int Cout, int IH, int IW, int ksize, int stride, size_t* bytes);
/* dw (OIHW) and optional db from the layer input x and the gradient g w.r.t. the conv output; both are clamped to
 * +-clip when clip > 0 (the per-parameter hook of yogo/model.py:76-77).  Deterministic (no float atomics).        */
int yogo_conv2d_wgrad_f32(const float* x, const float* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout,
                          int IH, int IW, int ksize, int stride, float clip, yogo_stream_t stream);

/* ---- first convolution: Cin = 1|3, uint8 or fp32 input (model_defns.py:34 + the cast at model.py:272-273) --------- */
int yogo_conv_first_stats_rows(int B, int IH, int IW, int stride, int* rows);
/* in_dtype: 0 = uint8, 1 = float32.  stats_part rows: [rows][Cout][2] */
int yogo_conv_first_fwd(const void* in, int in_dtype, const float* w_oihw, const float* bias, float* out, float* out_pre,
                        const float* chan_scale, float* stats_part, int B, int Cin, int Cout, int IH, int IW, int stride,
                        int act, yogo_stream_t stream);
/* partial gradients [rows][Cout][Cin*9 + 1] (last column = bias), rows from yogo_conv_first_wgrad_rows; finish with
 * yogo_partials_reduce */
int yogo_conv_first_wgrad_rows(int B, int IH, int IW, int stride, int* rows);
int yogo_conv_first_wgrad(const void* in, int in_dtype, const float* dy, float* part, int B, int Cin, int Cout, int IH,
                          int IW, int stride, yogo_stream_t stream);

/* ---- BatchNorm2d (model_defns.py:35,55,60): batch statistics, apply + activation, backward ------------------------ */
int yogo_bn_finalize(const float* part, int rows, int row_stride, int C, long long count, float eps, float momentum,
                     float* mean_out, float* invstd_out, float* running_mean, float* running_var,
                     long long* num_batches_tracked, yogo_stream_t stream);
/* yogo_bn_apply_act, yogo_bn_bwd: one grid row per (image, channel) plane, B * C <= 65535 (an argument error beyond) */
int yogo_bn_apply_act(const float* z, float* y, const float* mean, const float* invstd_or_var, int stat_is_var, float eps,
                      const float* gamma, const float* beta, int B, int C, int HW, int act, yogo_stream_t stream);
int yogo_bn_invstd(const float* var, float eps, float* invstd, int C, yogo_stream_t stream);
int yogo_bn_bwd_rows(int B, int HW, int* rows);
/* g: gradient w.r.t. the block OUTPUT; the activation derivative (act) is applied inside from the recomputed
 * pre-activation, then dz, dgamma, dbeta (clamped to +-clip when clip > 0) */
int yogo_bn_bwd(const float* g, const float* z, float* dz, const float* mean, const float* invstd, const float* gamma,
                const float* beta, int act, float* dgamma, float* dbeta, float* part, float* sums, int B, int C, int HW,
                int training, float clip, yogo_stream_t stream);
/* `part` is folded in place (used as scratch) */
int yogo_partials_reduce(float* part, int rows, int N, float clip, float* out, yogo_stream_t stream);
int yogo_channel_sum(const float* g, int B, int C, int HW, float clip, float* out, yogo_stream_t stream);

/* ---- box decode: YOGO.forward, yogo/model.py:277-313 ------------------------------------------------------------------ */
int yogo_decode_fwd(const float* raw, float* out, const float* cxs, const float* cys, int B, int P, int Sy, int Sx,
                    float anchor_w, float anchor_h, float width_multiplier, float height_multiplier, int inference,
                    yogo_stream_t stream);
int yogo_decode_bwd(const float* raw, const float* out, const float* gout, float* graw, int B, int P, int Sy, int Sx,
                    int inference, yogo_stream_t stream);

/* the same, gradient written as bf16 NCHW8c [B][2 * ceil(P / 16)][Sy][Sx][8] for the bf16 backward pass of the head convolution */
int yogo_decode_bwd_bf16(const float* raw, const float* out, const float* gout, void* graw8c, int B, int P, int Sy, int Sx,
                         int inference, yogo_stream_t stream);

/* ---- loss: YOGOLoss.forward, yogo/yogo_loss.py:38-129 (+ its autograd) ------------------------------------------------- */
int yogo_loss_workspace_bytes(int B, int Sy, int Sx, size_t* bytes);
/* loss_out: 4 device floats {total, iou_loss, objectness_loss, classification_loss}; grad = d total / d pred */
int yogo_loss_fwd_bwd(const float* pred, const float* label, float* grad, float* loss_out, void* workspace, int B, int P,
                      int Sy, int Sx, float no_obj_weight, float iou_weight, float classify_weight, float label_smoothing,
                      yogo_stream_t stream);

/* The trainer's fused form of the three calls above (yogo_decode_fwd + yogo_loss_fwd_bwd + yogo_decode_bwd_bf16) for TRAINING mode
 * (class logits pass through the decode): replaces YOGO.forward's decode (yogo/model.py:277-313), YOGOLoss.forward
 * (yogo/yogo_loss.py:38-129) and the autograd of both inside Trainer.train's step (yogo/train.py:309-322).  One pass over the
 * cells; the decoded prediction and its gradient never go to memory.  graw8c / loss_out / workspace as in the separate calls. */
int yogo_decode_loss_bwd_bf16(const float* raw, const float* label, const float* cxs, const float* cys, void* graw8c, float* loss_out,
                              void* workspace, int B, int P, int Sy, int Sx, float anchor_w, float anchor_h, float width_multiplier,
                              float height_multiplier, float no_obj_weight, float iou_weight, float classify_weight,
                              float label_smoothing, yogo_stream_t stream);

/* ---- post-process: format_preds, yogo/utils/prediction_formatting.py:23-93, batched over images ------------------------ */
int yogo_format_preds_workspace_bytes(int B, int Sy, int Sx, size_t* bytes);
/* out_rows [B][cap][P], out_cells [B][cap] (int64 cell index y*Sx+x), out_count [B] (int32).
 * box_format 0 = cxcywh, 1 = xyxy.  Row order per image is the reference's: descending max(class)*objectness
 * (ties: lower cell first) when iou_thresh > 0, cell order otherwise.                                                    */
int yogo_format_preds_batched(const float* pred, float* out_rows, long long* out_cells, int* out_count, void* workspace,
                              int B, int P, int Sy, int Sx, int cap, double obj_thresh, double iou_thresh, int box_format,
                              double min_class_confidence_threshold, yogo_stream_t stream);
/* The inference driver's fused form of yogo_decode_fwd + yogo_format_preds_batched (SURVEY.md 8(b) `decode_nms_batched`): `raw` is
 * the head's output BEFORE YOGO.forward's decode (yogo/model.py:277-313); the kernel decodes each value where it loads it, so the
 * decoded [B, 5+C, Sy, Sx] tensor that `yogo infer` hands from the model to format_preds (yogo/infer.py:45,73) never goes through
 * memory.  Rows, cells and counts are bit-identical to the two separate calls.  cxs / cys / anchor / multipliers / inference as
 * yogo_decode_fwd, the rest as yogo_format_preds_batched (same workspace query).                                              */
int yogo_decode_format_preds_batched(const float* raw, const float* cxs, const float* cys, float* out_rows, long long* out_cells,
                                     int* out_count, void* workspace, int B, int P, int Sy, int Sx, int cap, float anchor_w,
                                     float anchor_h, float width_multiplier, float height_multiplier, int inference,
                                     double obj_thresh, double iou_thresh, int box_format, double min_class_confidence_threshold,
                                     yogo_stream_t stream);
/* Eval-mode `model(x)` (yogo/model.py:275-313: self.model(x), then the decode) with the 1x1 head and the box decode in ONE launch
 * (SURVEY.md 8(b) `head1x1_decode_fwd`): x = the last 3x3 block's output, bf16 NCHW8c [B][Cin][Sy][Sx] (Cin a multiple of 16, <= 128),
 * packed = yogo_conv_bf16_pack(w [P][Cin][1][1], mode 0), bias [P] or null; out fp32 [B][P][Sy][Sx] = what yogo_conv2d_fwd_bf16 with an
 * fp32 output followed by yogo_decode_fwd writes, bit for bit -- the raw head output never goes through memory.  6 <= P <= 16.      */
int yogo_head1x1_decode_fwd_bf16(const void* x, const void* packed, const float* bias, float* out, const float* cxs, const float* cys,
                                 int B, int Cin, int P, int Sy, int Sx, float anchor_w, float anchor_h, float width_multiplier,
                                 float height_multiplier, int inference, yogo_stream_t stream);

/* ---- evaluation: prediction <-> label matching and the class statistics of `Metrics`, batched over images -------------------- */
/* format_preds_and_labels_v2 after its format_preds call (yogo/utils/prediction_formatting.py:287-330) for every image of a batch in
 * ONE launch, one workgroup per image: the label cells with label[0] != 0 in ascending cell order (:292-293), cost = 1 - box_iou in
 * fp32 (:297-299), scipy.optimize.linear_sum_assignment's shortest-augmenting-path solver in fp64 with its tie-breaking (:300), the
 * unmatched labels and rows (:309-323).  rows [B][cap][P] / counts [B] = yogo_format_preds_batched's output with box_format 1;
 * labels [B][6][Sy][Sx]; cap >= Sy*Sx.  Outputs at fixed strides (nothing depends on a host read): meta [B][8] int32 = {N labels,
 * M rows, n_pairs, n_missed, n_extra, status, every class score of the matched rows lies in [0, 1], 0}; pair_label / pair_pred
 * [B][cap] (ascending label index; indices into the compacted labels / the rows); un_label / un_pred [B][cap] ascending; lab_out
 * [B][cap][6] the compacted label rows.  status: 0 ok, 1 a cost is NaN or -inf, 2 infeasible (scipy's two ValueErrors); an image with
 * a status has no pairs and no unmatched entries.  The solver state is in LDS when N and M fit, else in the workspace. */
int yogo_match_workspace_bytes(int B, int Sy, int Sx, int cap, size_t* bytes);
int yogo_match_preds_labels_batched(const float* rows, const int* counts, const float* labels, int* meta, int* pair_label,
                                    int* pair_pred, int* un_label, int* un_pred, float* lab_out, void* workspace, int B, int P, int Sy,
                                    int Sx, int cap, yogo_stream_t stream);
/* PredictionLabelMatch.concat over the images (prediction_formatting.py:183-204): preds [K][P], labels [K][6], missed [Km][6],
 * extra [Ke][P] with K / Km / Ke the sums of n_pairs / n_missed / n_extra (outputs of a zero size may be null). */
int yogo_match_gather(const float* rows, const float* lab_out, const int* meta, const int* pair_label, const int* pair_pred,
                      const int* un_label, const int* un_pred, float* preds, float* labels, float* missed, float* extra, int B, int P,
                      int cap, long long K, long long Km, long long Ke, yogo_stream_t stream);
/* What Metrics.update adds per batch (yogo/metrics.py:113-158, include_background=False) from the match output, without a host read:
 * acc (int64, laid out as yogo_metrics_state_layout reports) = confmat [C][C] (first argmax of the C class scores), pos [C], n, missed-by-class [C],
 * extra-by-class [C], total true objects, bin_count [nbins], bin_acc [nbins], hist [T+1][C][2] (k = #{roc_thresholds <= p}, class,
 * is-target; the binned ROC's tp / fp at threshold t are the sums over k > t), mAP row count, images with status 1, with status 2.
 * Probabilities in fp64: the scores, or their softmax unless every class score of the batch's matched rows lies in [0, 1]
 * (torchmetrics' rule).  bin_conf [nbins] fp64 += the confidences per calibration bin, summed in a fixed order through partial
 * [B][nbins] (no floating-point atomics: two runs give the same bits).  roc_thresholds [T] / cal_edges [nbins + 1]: the doubles of
 * torch.linspace, on the device.  map_rows [map_cap][11] fp32 or null: per pair the row's box, objectness, first-argmax class, the
 * label's box and class, appended at the running count (rows past map_cap are counted, not written). */
/* offsets (HOST pointer, 12 values): where confmat, pos, n, missed, extra, total, bin_count, bin_acc, hist, the mAP row count and the
 * two status counts start in acc, then the number of int64 words of acc */
int yogo_metrics_state_layout(int C, int T, int nbins, long long* offsets);
int yogo_metrics_accumulate(const float* rows, const float* lab_out, const int* meta, const int* pair_label, const int* pair_pred,
                            const int* un_label, const int* un_pred, const double* roc_thresholds, int T, const double* cal_edges,
                            int nbins, long long* acc, double* bin_conf, double* partial, float* map_rows, long long map_cap, int B,
                            int P, int cap, yogo_stream_t stream);

/* ---- inference outputs kept on the device: `yogo infer --device-outputs` (yogo_amd/pred_sink.py) ------------------------------- */
/* What predict's output stage does per batch with the kept rows (yogo/infer.py:39-124,360-380), without a host read: rows [B][cap][P] /
 * counts [B] = the output of yogo_format_preds_batched or yogo_decode_format_preds_batched (entries past counts[b] are never read; a
 * counts[b] outside [0, cap] is clamped).  state (int64, laid out as yogo_pred_sink_state_layout reports) = records in the arena, images
 * in img_counts, records dropped, image entries dropped, class_counts [C] (C = P - 5).  Record k of image b goes to row
 * state.records + sum(counts[:b]) + k of arena [arena_cap][reclen], counts[b] to img_counts [img_cap] at state.images + b (int32);
 * both totals then advance.  What does not fit is counted as dropped and not written.
 * mode 0: reclen = 8 + C, the columns of format_to_numpy (yogo/utils/prediction_formatting.py:96-156): first_img_id + b, x1*img_w,
 * y1*img_h, x2*img_w, y2*img_h (one fp32 multiply each), objectness, first-argmax class, its score, the C scores; C <= 255 (the
 * reference holds the class in a uint8).  mode 1: reclen = P, the row itself.  arena null: nothing is compacted and the totals stay
 * (mode, img_counts, workspace are not used; count_classes must be 1).
 * count_classes 1: class_counts[first argmax] += 1 for every kept row whose maximum class score is > 0 (a NaN is the maximum and is
 * not > 0) -- count_cells_for_formatted_preds, yogo/infer.py:90-124; integer adds only.  workspace: yogo_pred_sink_workspace_bytes. */
/* offsets (HOST pointer, 6 values): where the record total, the image total, the dropped records, the dropped image entries and
 * class_counts start in state, then the number of int64 words of state */
int yogo_pred_sink_state_layout(int C, long long* offsets);
int yogo_pred_sink_workspace_bytes(int B, size_t* bytes);
int yogo_pred_sink_append(const float* rows, const int* counts, int B, int cap, int P, int mode, int count_classes,
                          long long first_img_id, int img_h, int img_w, long long* state, float* arena, long long arena_cap,
                          int* img_counts, long long img_cap, void* workspace, yogo_stream_t stream);
/* The prediction files of --save-preds (yogo/infer.py:52-55) as text, written on the device.  The definition is
 * prediction_rows_to_text (yogo_amd/utils/prediction_formatting.py): per row "<class> <cx> <cy> <w> <h>" -- class =
 * max(range(C), key=scores.__getitem__) (the first maximum under ">": a NaN never displaces the current best), the four numbers as
 * repr(float(numpy.float32(v))), shortest round-trip decimals (yogo_amd/csrc/float_text.h) -- the rows of an image joined by "\n" with
 * no trailing newline, an image without rows an empty text.  records [n][P] fp32 in image order and img_counts [images] int32 = what a
 * mode-1 sink holds at drain time.  text [text_cap] receives the images' texts back to back, img_offsets [images + 1] (int64) where each
 * starts (image k is text[img_offsets[k] : img_offsets[k + 1]]), total (ONE device int64) the byte count NEEDED: the text is complete
 * iff 0 <= total <= text_cap, and nothing is ever stored at or past text_cap (text may be null when text_cap is 0: a measuring run).
 * img_counts is not trusted: a negative entry or a sum other than n gives total = -1, and text / img_offsets are not written.
 * n = 0 launches nothing (offsets and total become 0 by stream-ordered memsets; img_counts is not read); n > 0 with images = 0 is an
 * argument error.  n, images <= INT_MAX.  workspace: 8-byte aligned, yogo_pred_text_bound's workspace_bytes. */
/* HOST pointers: text_bytes = a capacity that no records of n_records rows with P - 5 class scores can exceed (at most 1 + the digits
 * of C - 1 + 4 * 25 bytes per row), workspace_bytes = the scratch of yogo_pred_text_format (one byte per record, 8 per image and per
 * 256 records) */
int yogo_pred_text_bound(long long n_records, long long images, int P, size_t* text_bytes, size_t* workspace_bytes);
int yogo_pred_text_format(const float* records, long long n, int P, const int* img_counts, long long images, char* text,
                          long long text_cap, long long* img_offsets, long long* total, void* workspace, yogo_stream_t stream);

/* ---- bf16 path: the bf16-autocast forward of `yogo infer` (yogo/infer.py:313-317) and half-precision training
 * (yogo/train.py:315-318, --half) -------------------------------------------------------------------------------------------
 * Activations and activation gradients in "NCHW8c" = [B][C/8][H][W][8] bf16 (C padded to a multiple of 16; padding
 * channels hold zeros); weights, BatchNorm statistics, parameter gradients, optimiser state stay fp32.
 * Inference folds eval-mode BatchNorm into `scale` (weights) and `bias` on the caller's side.                               */
int yogo_bf16_channel_blocks(int C);
/* mode 0: forward packing (optional per-output-channel scale); mode 1: dgrad packing (roles swapped, taps flipped);
 * mode 2: dgrad packing for a stride-2 3x3 convolution (as 1, tap slices in output-parity-class order) */
int yogo_conv_bf16_packed_bytes(int Cin, int Cout, int ksize, int mode, size_t* bytes);
int yogo_conv_bf16_pack(const float* w_oihw, const float* scale, void* packed, int Cin, int Cout, int ksize, int mode,
                        yogo_stream_t stream);
int yogo_conv2d_fwd_bf16_stats_shape(int B, int Cin, int Cout, int IH, int IW, int ksize, int stride, int* rows, int* mpad);
/* Plan (no counterpart in the reference; cuDNN picks its algorithm behind torch.backends.cudnn.benchmark, yogo/train.py:36): the 3x3
 * bf16 convolutions with 128 GEMM rows and 64 / 128 / ... contraction channels (forward of yogo/model_defns.py:49-65's 128-channel
 * blocks and their data gradients) run on the persistent wavefront-specialised kernels (conv_bf16_ws_kernel; 8 wavefronts per CU: 4
 * compute, 4 load / store), everything else on the tiled conv_bf16_kernel.  The two families agree bit for bit where the tiled plan
 * also steps the contraction in 16-channel chunks (every shape of the training step), within one bf16 ulp otherwise.  The library has
 * no run-time plan switch and no mutable global state besides its lazily-loaded module handles and the launch log: the A/B switches
 * used by tests/ and tools/ (yogo_hook_*) exist only in libyogo_hip_hooks.so, which the package never loads: the product's object files
 * with the one host-only unit that owns every plan switch (csrc/plan_switches.hip) compiled under -DYOGO_TEST_HOOKS (build.sh). */
/* y = chan_scale * act(conv(x) + bias); out: bf16 NCHW8c, or fp32 NCHW when out_f32 != NULL (the head);
 * stats_part (optional): BatchNorm partial (sum, sumsq) of the fp32 pre-activation */
int yogo_conv2d_fwd_bf16(const void* in, const void* packed, const float* bias, void* out, float* out_f32,
                         const float* chan_scale, float* stats_part, int B, int Cin, int Cout, int IH, int IW, int ksize,
                         int stride, int act, yogo_stream_t stream);
/* as above plus a second bf16 NCHW8c output out_pre = conv + bias before the activation (SiLU blocks without BatchNorm keep it:
 * the activation derivative of yogo/model_defns.py's nn.SiLU is a function of the pre-activation) */
int yogo_conv2d_fwd_bf16_pre(const void* in, const void* packed, const float* bias, void* out, void* out_pre,
                             const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ksize, int stride, int act,
                             yogo_stream_t stream);
/* yogo_conv_bf16_pack for a list of tensors in one launch (a training step repacks every layer twice).  table: device int64
 * [n][8] = {w pointer, scale pointer or 0, packed pointer, Cin, Cout, ksize, mode, first block}; entry k owns
 * yogo_conv_bf16_pack_blocks blocks starting at its first block; total_blocks = their sum */
int yogo_conv_bf16_pack_blocks(int Cin, int Cout, int ksize, int mode, int* blocks);
int yogo_conv_bf16_pack_multi(const void* table, int n, int total_blocks, yogo_stream_t stream);
/* LeakyReLU sign map of a bf16 NCHW8c tensor: [B][2][H][W][Cpad/16] bytes (Cpad = C rounded up to 32 / 64 / a multiple of 128
 * for C <= 32 / <= 64 / more); byte (h, pixel, q), bit i + 4e = (channel 4h + i of channel block 2q + e > 0), h, e in {0, 1},
 * i < 4; bytes of channel blocks beyond kb(C) are unspecified -- all the data gradient needs of a LeakyReLU block's output (torch's
 * leaky_relu_backward reads the whole tensor), at 1/16 of its bytes */
int yogo_bf16_signs_bytes(int B, int C, int H, int W, size_t* bytes);
/* yogo_conv2d_fwd_bf16 (bf16 output) that also writes the sign map of its output */
int yogo_conv2d_fwd_bf16_signs(const void* in, const void* packed, const float* bias, void* out, void* signs,
                               const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ksize, int stride, int act,
                               yogo_stream_t stream);
/* Two LeakyReLU blocks without BatchNorm in one call (yogo/model_defns.py:39-46, blocks 2 and 3 of base_model: Conv2d(16, 32, 3, padding=1)
 * and Conv2d(32, 64, 3, stride=2, padding=1), each with LeakyReLU and -- the second -- Dropout2d): out1 / signs1 = yogo_conv2d_fwd_bf16_signs
 * (in, packed1, bias1, scale1; C0 -> C1, stride 1), out2 / signs2 = the same of out1 (packed2, bias2, scale2; C1 -> C2, stride 2), every
 * stored byte identical to the two calls.  Where yogo_conv2d_fwd_bf16_signs_pair_eligible returns 1 (C0 = 16, C1 = 32 < C2 <= 64, extents
 * below 2^31) and act is LeakyReLU the pair runs as ONE launch whose second layer reads out1 from LDS instead of memory; otherwise as the
 * two launches.  out1 and signs1 are written either way (the backward pass reads them). */
int yogo_conv2d_fwd_bf16_signs_pair_eligible(int B, int C0, int C1, int C2, int IH, int IW);
int yogo_conv2d_fwd_bf16_signs_pair(const void* in, const void* packed1, const float* bias1, void* out1, void* signs1,
                                    const float* scale1, const void* packed2, const float* bias2, void* out2, void* signs2,
                                    const float* scale2, int B, int C0, int C1, int C2, int IH, int IW, int act,
                                    yogo_stream_t stream);
/* yogo_conv2d_dgrad_bf16 for a LeakyReLU reference given as its sign map: dx = conv_transpose(dy) * (bit ? 1 : 0.01) * chan_scale.
 * Contract against yogo_conv2d_dgrad_bf16 with the bf16 reference tensor: the same bits wherever both run on the same kernel; the
 * stride-2 3x3 shapes conv_bf16_s2d_direct_kernel takes (<= 32 or 65..128 input channels of the forward convolution) step the
 * contraction 16 channels at a time where the tiled kernel takes 32 / 64: equal to ONE bf16 rounding step on < 0.5 % of the values
 * (tests/test_gpu_bf16.py, tests/test_gpu_ws.py).  The same one-step contract holds between conv_bf16_ws16_kernel (the plain-epilogue
 * stride-1 launches with 128 output channels and a multiple of 64 input channels: two 16-channel chunks summed inside one MFMA) and
 * the 32x32x16 kernels. */
int yogo_conv2d_dgrad_bf16_signs(const void* dy, const void* packed_dgrad, void* dx, const void* signs,
                                 const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ksize, int stride,
                                 yogo_stream_t stream);
/* dx = conv_transpose(dy) * act'(act_ref) * chan_scale, everything bf16 NCHW8c; (IH, IW) = forward INPUT dims */
int yogo_conv2d_dgrad_bf16(const void* dy, const void* packed_dgrad, void* dx, const void* act_ref, int ref_act,
                           const float* chan_scale, int B, int Cin, int Cout, int IH, int IW, int ksize, int stride,
                           yogo_stream_t stream);
/* fp32 dw/db from bf16 NCHW8c x and g (exact fp32 MFMA on the widened values); workspace as yogo_conv2d_wgrad_f32 */
int yogo_conv2d_wgrad_bf16in(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout,
                             int IH, int IW, int ksize, int stride, float clip, yogo_stream_t stream);
/* the same on the bf16 matrix cores (contraction over pixels through transposed LDS reads), fp32 accumulation */
int yogo_conv2d_wgrad_bf16_workspace_bytes(int B, int Cin, int Cout, int IH, int IW, int ksize, int stride, size_t* bytes);
int yogo_conv2d_wgrad_bf16(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout,
                           int IH, int IW, int ksize, int stride, float clip, yogo_stream_t stream);
/* ... with the split-K reduction deferred (ABI 5): recorded in `queue` and run by yogo_wgrad_reduce_flush together with every other
 * recorded one -- one launch for the weight gradients of a whole backward pass (the per-layer launches are ~21 us each, mostly launch and
 * tail latency).  dw / db / workspace stay valid until the flush; results are bit-identical to yogo_conv2d_wgrad_bf16.  A queue holds up
 * to 16 reductions (a 17th flushes first, on the stream of the call that records it) and belongs to one host thread AND one stream:
 * record and flush a queue on the same stream. */
int yogo_wgrad_reduce_queue_create(void** queue_out);
int yogo_wgrad_reduce_queue_destroy(void* queue);
int yogo_wgrad_reduce_queue_reset(void* queue);   /* forget the recorded reductions without running them */
int yogo_wgrad_reduce_flush(void* queue, yogo_stream_t stream);
int yogo_conv2d_wgrad_bf16_deferred(const void* x, const void* g, float* dw, float* db, void* workspace, int B, int Cin, int Cout, int IH,
                                    int IW, int ks, int stride, float clip, void* queue, yogo_stream_t stream);
int yogo_conv_first_fwd_bf16(const void* in, int in_dtype, const float* w, const float* bias, void* out, int B, int Cin,
                             int Cout, int IH, int IW, int stride, int act, yogo_stream_t stream);
int yogo_conv_first_fwd_train_bf16(const void* in, int in_dtype, const float* w, const float* bias, void* out_bf16,
                                   const float* chan_scale, float* stats_part, int B, int Cin, int Cout, int IH, int IW,
                                   int stride, int act, yogo_stream_t stream);
int yogo_conv_first_wgrad_bf16g(const void* in, int in_dtype, const void* dy_bf16, float* part, int B, int Cin, int Cout,
                                int IH, int IW, int stride, yogo_stream_t stream);
/* Layer-0 backward in one pass: BatchNorm backward (model_defns.py:35) + activation derivative + weight gradient of the first
 * convolution; g = gradient w.r.t. the block output, z = saved conv output, both bf16 NCHW8c.  part: rows
 * (yogo_conv_first_wgrad_rows) x cols (yogo_conv_first_bn_wgrad_cols) floats; then yogo_partials_reduce(part, rows, cols, 0,
 * sums) and yogo_conv_first_bn_wgrad_finalize (dw OIHW, dgamma, dbeta, clamped to +-clip). */
int yogo_conv_first_bn_wgrad_cols(int Cin, int Cout, int* cols);
int yogo_conv_first_bn_wgrad_bf16(const void* in, int in_dtype, const void* g, const void* z, const float* mean,
                                  const float* invstd, const float* gamma, const float* beta, float* part, int B, int Cin,
                                  int Cout, int IH, int IW, int stride, int act, yogo_stream_t stream);
int yogo_conv_first_bn_wgrad_finalize(const float* sums, const float* mean, const float* invstd, const float* gamma,
                                      const float* w_oihw, float* dw, float* dgamma, float* dbeta, int B, int Cin, int Cout,
                                      int IH, int IW, int stride, int training, float clip, yogo_stream_t stream);
int yogo_bn_apply_act_bf16(const void* z, void* y, const float* mean, const float* invstd_or_var, int stat_is_var, float eps,
                           const float* gamma, const float* beta, int B, int C, int HW, int act, yogo_stream_t stream);
int yogo_bn_bwd_bf16_rows(int B, int HW, int* rows);
/* batch statistics of a stored bf16 NCHW8c tensor: part [rows][C][2] (rows = yogo_bn_bwd_bf16_rows), then yogo_bn_finalize */
int yogo_bn_stats_bf16(const void* z, float* part, int B, int C, int HW, yogo_stream_t stream);
int yogo_bn_bwd_bf16(const void* g, const void* z, void* dz, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, int act, float* dgamma, float* dbeta, float* part, float* sums, int B, int C, int HW,
                     int training, float clip, yogo_stream_t stream);
/* ... of the block under a 1x1 convolution with P <= 16 outputs (the detection head, yogo/model.py:150-155) WITHOUT that convolution's data
 * gradient in memory (ABI 7): gh = gradient w.r.t. the head's output (bf16 NCHW8c [B][2][HW], channels >= P zero), head_w = the head's
 * weights [P][C]; g = bf16(sum_k gh[k] * bf16(w[k][c])) is computed inside both sweeps (one MFMA per 16 pixels x 16 channels).  C a
 * multiple of 16; dz must not alias gh.  Replaces the head's yogo_conv2d_dgrad_bf16 + yogo_bn_bwd_bf16. */
int yogo_bn_bwd_bf16_head(const void* gh, const float* head_w, int P, const void* z, void* dz, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, int act, float* dgamma, float* dbeta, float* part, float* sums, int B,
                          int C, int HW, int training, float clip, yogo_stream_t stream);
/* fp32 NCHW <-> bf16 NCHW8c (C padded to a multiple of 16, padding lanes written as zero / not read back); the rounding is to nearest
 * even, NaN stays NaN.  B * 2 * ceil(C / 16) <= 65535 (an argument error beyond), as for every bf16 entry point above. */
int yogo_nchw_f32_to_bf16_8c(const float* in, void* out, int B, int C, int HW, yogo_stream_t stream);
int yogo_bf16_8c_to_nchw_f32(const void* in, float* out, int B, int C, int HW, yogo_stream_t stream);

/* ---- layer 0 of the bf16 training path on the matrix cores (uint8 image, Cin = 1, Cout <= 16, stride 2, even H and W):
 * Conv2d + the uint8 -> float cast (yogo/model_defns.py:34, yogo/model.py:272) and the BatchNorm2d + activation behind it
 * (model_defns.py:35).  Weights are rounded to bf16 inside (autocast, yogo/train.py:315-318).  Outputs, each optional:
 * stats_part = partial (sum, sumsq) of conv + bias in fp32, [rows][16][2] with rows from yogo_conv_first_mfma_stats_rows ->
 * yogo_bn_finalize(part, rows, 16, ...); z = conv + bias, bf16 NCHW8c; y = act((z - mean) * invstd * gamma + beta), bf16
 * NCHW8c; without y the activation is applied to z (inference, BatchNorm folded into w / bias).  Training: statistics (this
 * kernel or yogo_conv_first_gram), then z + y in one sweep instead of conv + a separate BatchNorm pass over the activations. */
int yogo_conv_first_mfma_supported(int in_dtype, int Cin, int Cout, int IH, int IW, int stride);
int yogo_conv_first_mfma_stats_rows(int B, int IH, int IW, int* rows);
int yogo_conv_first_mfma(const void* in, const float* w, const float* bias, void* z, void* y, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, float* stats_part, int B, int Cout, int IH,
                         int IW, int act, yogo_stream_t stream);

/* Batch statistics of that layer WITHOUT the convolution: z = w . patch + b is linear in the 3x3 patch, so the statistics of all
 * channels follow from P = sum patch (9) and G = sum patch (x) patch (9 x 9) over the batch -- accumulated exactly in integers.
 * part: scratch, yogo_conv_first_gram_rows x 54 uint32; gram: double[90], gram_f32: float[90] (P[9], then G[9][9]).
 * yogo_bn_stats_from_gram = yogo_bn_finalize on those sums (w rounded to bf16 as the convolution does); the backward pass
 * reuses gram_f32 (yogo_conv_first_bn_wgrad_bf16_xg / _finalize_xg) instead of sweeping the image again. */
int yogo_conv_first_gram_rows(int B, int IH, int IW, int* rows);
int yogo_conv_first_gram(const void* in, void* part, double* gram, float* gram_f32, int B, int IH, int IW, yogo_stream_t stream);
int yogo_bn_stats_from_gram(const double* gram, const float* w, const float* bias, int Cout, long long count, float eps,
                            float momentum, float* mean_out, float* invstd_out, float* running_mean, float* running_var,
                            long long* num_batches_tracked, yogo_stream_t stream);
int yogo_conv_first_bn_wgrad_bf16_xg(const void* in, int in_dtype, const void* g, const void* z, const float* mean,
                                     const float* invstd, const float* gamma, const float* beta, float* part, int B, int Cin,
                                     int Cout, int IH, int IW, int stride, int act, yogo_stream_t stream);
int yogo_conv_first_bn_wgrad_finalize_xg(const float* sums, const float* gram, const float* mean, const float* invstd,
                                         const float* gamma, const float* w_oihw, float* dw, float* dgamma, float* dbeta, int B,
                                         int Cin, int Cout, int IH, int IW, int stride, int training, float clip,
                                         yogo_stream_t stream);
/* The same pair of sweeps WITHOUT the layer's conv output z in memory (ABI 5).  What the backward pass needs of z is (a) the sign of
 * the BatchNorm output for the LeakyReLU derivative and (b) sum g * xhat, which is linear in z = W . patch and follows from the
 * weight-gradient sums themselves.  yogo_conv_first_mfma_signs = yogo_conv_first_mfma that also writes (a) as a bit map, signs =
 * [B][OH*OW][2] bytes (byte h of a pixel: bit i = channel 4h + i, bit 4 + i = channel 8 + 4h + i; z may then be NULL);
 * yogo_conv_first_bn_wgrad_bf16_xs reads it in place of z (_xs_supported: uint8 one-channel image, stride 2, even sizes, Cout 8 or
 * 16, ACT_NONE / ACT_LEAKY, no conv bias); yogo_conv_first_bn_wgrad_finalize_xs derives (b); w_oihw there = the bf16-rounded weights
 * the forward pass multiplied with.  Replaces the same reference lines as the _xg pair (model_defns.py:34-35 under autograd). */
int yogo_conv_first_mfma_signs(const void* in, const float* w, const float* bias, void* z, void* y, void* signs, const float* mean,
                               const float* invstd, const float* gamma, const float* beta, int B, int Cout, int IH, int IW, int act,
                               yogo_stream_t stream);
int yogo_conv_first_bn_wgrad_xs_supported(int in_dtype, int Cin, int Cout, int IH, int IW, int stride, int act);
/* (both sweeps take two adjacent pixels per lane where the output width is even, one otherwise)
 * Image alignment: no sweep of the yogo_conv_first_bn_wgrad_bf16* family loads wider than `in` is aligned.  The two-pixel sweep reads
 * aligned dwords and runs only when in % 4 == 0; the one-pixel sweeps read 16-bit words and need in % 2 == 0; _bf16 and _bf16_xg fall
 * back to their byte-wise kernel for an odd address (same sums).  _xs has no byte-wise route: an image at an odd address is REFUSED
 * (YOGO_ERR_ARG, "aligned to 2 bytes"); at in % 4 == 2 it runs the one-pixel sweep. */
int yogo_conv_first_bn_wgrad_bf16_xs(const void* in, int in_dtype, const void* g, const void* signs, const float* mean,
                                     const float* invstd, const float* gamma, const float* beta, float* part, int B, int Cin,
                                     int Cout, int IH, int IW, int stride, int act, yogo_stream_t stream);
int yogo_conv_first_bn_wgrad_finalize_xs(const float* sums, const float* gram, const float* mean, const float* invstd,
                                         const float* gamma, const float* w_oihw, float* dw, float* dgamma, float* dbeta, int B,
                                         int Cin, int Cout, int IH, int IW, int stride, int training, float clip,
                                         yogo_stream_t stream);
/* Layer 1's data gradient and the sweep of yogo_conv_first_bn_wgrad_bf16_xs in ONE launch (ABI 7): the gradient w.r.t. layer 0's output
 * is folded into layer 0's backward sums tile by tile and never written (layer 0 has no data gradient of its own).  g = gradient
 * w.r.t. layer 1's conv output, bf16 NCHW8c [B][Cout1 / 8][H][W]; packed = layer 1's yogo_conv_bf16_pack mode-1 packing; image = uint8
 * [B][2H][2W]; signs as above (NULL with ACT_NONE); part: rows (yogo_conv2d_dgrad_first_bwd_rows, on the current device) x cols
 * (yogo_conv_first_bn_wgrad_cols) floats; finish with yogo_partials_reduce and yogo_conv_first_bn_wgrad_finalize_xs exactly as after the
 * unfused sweep.  _supported: 3x3 stride-1 layer 1 with 16 -> 32 channels, even W.  Results agree with yogo_conv2d_dgrad_bf16 followed by
 * yogo_conv_first_bn_wgrad_bf16_xs to fp32 rounding of the sums (every element is rounded to bf16 as the stored gradient would have been).
 * Replaces autograd of yogo/model_defns.py:34-41 (the backward of the first two blocks of base_model). */
int yogo_conv2d_dgrad_first_bwd_supported(int Cmid, int Cout1, int H, int W, int B, int act0);
int yogo_conv2d_dgrad_first_bwd_rows(int B, int H, int W, int with_wgrad, int* rows);
int yogo_conv2d_dgrad_bf16_first_bwd(const void* g, const void* packed, const void* image, const void* signs, float* part, int B, int Cmid,
                                     int Cout1, int H, int W, int act0, yogo_stream_t stream);
/* ... and layer 1's WEIGHT gradient in the same sweep (it reads the same g; x = layer 1's input = layer 0's output, bf16 NCHW8c): dw (OIHW)
 * and db (may be NULL) clamped to +-clip, as yogo_conv2d_wgrad_bf16 / _deferred deliver them (queue: NULL = reduce now, else a
 * yogo_wgrad_reduce_queue); part rows: yogo_conv2d_dgrad_first_bwd_rows(..., 1, ...).  Replaces autograd of model_defns.py:34-41 except
 * layer 1's own data-gradient input. */
int yogo_conv2d_dgrad_wgrad_first_bwd_workspace_bytes(int B, int H, int W, size_t* bytes);
int yogo_conv2d_dgrad_wgrad_bf16_first_bwd(const void* g, const void* packed, const void* x, const void* image, const void* signs, float* part,
                                           float* dw, float* db, void* workspace, int B, int Cmid, int Cout1, int H, int W, int act0,
                                           float clip, void* queue, yogo_stream_t stream);

/* ---- data-parallel exchange over RCCL / xGMI (replaces torch DDP: init_process_group("nccl") + DistributedDataParallel,
 * yogo/train.py:155-159; gradient all-reduce overlapped with backward, buffers broadcast from rank 0).  One process per GPU.
 * librccl.so is opened lazily.  yogo_comm_unique_id fills a HOST buffer of yogo_comm_unique_id_bytes() bytes on rank 0; the host
 * hands it to every rank (any rendez-vous) and each rank calls yogo_comm_init (collective).  The all-reduce is an in-place SUM
 * of fp32 values enqueued on `stream`; the mean's 1 / world is folded into yogo_adamw_step (grad_scale). */
int yogo_comm_unique_id_bytes(void);
int yogo_comm_unique_id(void* id_out_host);
int yogo_comm_init(int rank, int world, const void* unique_id_host, void** comm_out);
int yogo_comm_allreduce_flat(void* comm, float* buf, size_t count, yogo_stream_t stream);
int yogo_comm_broadcast_flat(void* comm, void* buf, size_t bytes, int root, yogo_stream_t stream);
int yogo_comm_destroy(void* comm);

/* ---- the step in front of the path: label rasteriser and batch flips ----------------------------- */
/* format_labels_tensor, yogo/data/yogo_dataset.py:24-46, for a whole batch.  labels: [N][5] fp32 rows (class, x1, y1, x2, y2),
 * or (class, xc, yc, w, h) with box_format = 1 (converted as label_file_to_tensor does, :132), all images back to back;
 * offsets: [B + 1] int32 row ranges; out: [B][6][Sy][Sx] fp32 = (mask, x1, y1, x2, y2, class), written completely; a later
 * label of a cell overwrites an earlier one, negative cell indices wrap once (Python indexing).  status: one device int32 the
 * caller zeroes; set to 1 + the row index of a label whose cell is outside the grid (IndexError in the reference). */
int yogo_labels_rasterize(const float* labels, const int* offsets, float* out, int* status, int B, int Sx, int Sy,
                          int box_format, yogo_stream_t stream);
/* RandomHorizontalFlipWithBBs + RandomVerticalFlipWithBBs, yogo/data/data_transforms.py:51-98, applied to a batch in one pass
 * (the caller draws the decisions).  img: [B][C][H][W], elem_bytes 1 (uint8) or 4 (float32); lab: [B][6][Sy][Sx] fp32; out of
 * place; either pair may be NULL.  Box coordinates become 1 - x in EVERY cell, as in the reference. */
int yogo_flip_batch(const void* img_in, void* img_out, int elem_bytes, const float* lab_in, float* lab_out, int B, int C, int H,
                    int W, int Sy, int Sx, int hflip, int vflip, yogo_stream_t stream);

/* ---- thumbnail ("blob") augmentation, yogo/data/blobgen.py:208-263 (BlobDataset.__getitem__), S images per call ----------
 * Thumbnails: atlas = every kept thumbnail's uint8 pixels back to back (row-major h x w); table = [T][5] int32 (atlas offset,
 * h, w, class, shade), shade = blobgen.py:168-179 computed by the caller.  Every draw is a counter-based hash of
 * (seed, epoch, indices[s], slot, kind, try): the exact rule is at the top of yogo_amd/csrc/blobgen.hip.  Three steps:
 *   place      -> boxes [S][n][4] int32 (thumbnail, x, y, flips: bit 0 horizontal, bit 1 vertical), rows [S][n][5] fp32
 *                 (class, x / W, y / H, (x + w) / W, (y + h) / H) in placement order, counts [S], background [S]; entries past
 *                 counts[s] are zero.  n <= yogo_blobgen_max_n.  blobgen.py:140-160 (draws), :181-206 (100 tries, first try
 *                 that intersects no accepted box), :210-249 (background = truncated mean shade of all n draws, flips, labels)
 *   compose    -> images into rows positions[0 .. S) of out [B][1][H][W]: elem_bytes 1 = uint8, 4 = fp32 pixel / 255
 *                 (normalize_images, blobgen.py:261-262).  W <= 4096.  Deterministic, one store per output element.
 *   label_rows -> the placed rows as one flat list flat [S * n][5] with offsets [S + 1], the input of yogo_labels_rasterize
 *                 (box_format 0, xyxy) -- format_labels_tensor at blobgen.py:259 */
int yogo_blobgen_max_n(int* n);
int yogo_blobgen_place(const int* table, int num_thumbnails, const int* indices, int S, int n, int H, int W, long long seed,
                       long long epoch, int* boxes, float* rows, int* counts, int* background, yogo_stream_t stream);
int yogo_blobgen_compose(const unsigned char* atlas, long long atlas_bytes, const int* table, const int* boxes, const int* counts,
                         const int* background, const int* positions, int S, int n, int H, int W, void* out, int elem_bytes,
                         yogo_stream_t stream);
int yogo_blobgen_label_rows(const float* rows, const int* counts, int S, int n, float* flat, int* offsets, yogo_stream_t stream);

/* ---- decoded images resident in HBM (yogo_amd/image_cache.py, `yogo train --device-image-cache GIB`) ----------------------
 * cache: [S][C][H][W] uint8, the images of split indices 0 .. S-1 decoded once; slots: [B] int32 device; out: [B][C][H][W],
 * uint8 (out_fp32 = 0) or fp32 (out_fp32 = 1).  For every b with slots[b] >= 0, row b of out = cache[slots[b]], as uint8 or as
 * fp32 x / 255 bit-identical to torch's CPU uint8_tensor / 255 (normalize_images).  Rows with slots[b] < 0 are not touched
 * (uploaded rows, blob images); a slot >= S is skipped too, but the caller checks slots < S before the launch.  B <= 65535.
 * One HBM-bound pass, 16-byte accesses when C * H * W is a multiple of 16 and both buffers are 16-byte aligned. */
int yogo_image_cache_gather(const unsigned char* cache, int S, const int* slots, int B, int C, int H, int W, void* out, int out_fp32,
                            yogo_stream_t stream);

/* ---- zarr image stacks for inference (yogo_amd/zarr_feed.py, `yogo infer --path-to-zarr`) ---------------------------------
 * What the reference does per image on the host -- zarr_store[:, :, idx][None], CenterCrop, / 255
 * (yogo/data/image_path_dataset.py:115-126, yogo/infer.py:221-226) -- as one launch per batch over decoded chunks.
 * staged: staged_bytes of device memory, 16-byte aligned, holding whole decoded uint8 chunks of shape (ch, cw, cn) in C
 * (order_f = 0) or F (order_f = 1) order, each at a 16-byte aligned offset.  tile_off: [B][gh][gw] int64 device, the offset of
 * the chunk with tile (ty, tx) of batch row b's frame; a negative offset (the key is absent from the store), or one whose
 * chunk would not lie inside staged, makes the tile read as `fill`.  tile_k: [B] int32 device, the frame's position on the
 * chunk's innermost axis (idx % cn; the caller checks 0 <= tile_k < cn, a value outside reads as fill).  gh = ceil(H / ch),
 * gw = ceil(W / cw).  out: [B][1][OH][OW] uint8 (out_fp32 = 0) or fp32 x / 255 bit-identical to torch's CPU uint8_tensor / 255
 * (out_fp32 = 1): out[b][0][oy][ox] = frame_b[top + oy][left + ox], 1 <= OH <= H - top, 1 <= OW <= W - left (CenterCrop:
 * top = int(round((H - OH) / 2.0)), likewise left).  B <= 65535, H, W <= 65535.  Paths (named in the launch log): rows (C order,
 * cn == 1; 16-byte accesses when every segment is 16-byte aligned, else byte-wise), deinterleave (C order, 1 < cn <= 1024;
 * consecutive batch rows with one tile offset are served by one read of the chunk), gather (F order, or C order with cn > 1024; byte-wise). */
int yogo_zarr_unpack(const unsigned char* staged, long long staged_bytes, const long long* tile_off, const int* tile_k, int B, int gh,
                     int gw, int ch, int cw, int cn, int order_f, int fill, int H, int W, int top, int left, int OH, int OW, void* out,
                     int out_fp32, yogo_stream_t stream);
/* The blocks of Blosc-compressed chunks (zarr's default compressor), decoded on the device in front of yogo_zarr_unpack
 * (yogo_amd/blosc.py parses the chunk headers on the host; launched from yogo_amd/device_decode.py, as yogo_inflate_zlib is).  src: src_bytes of device memory holding stored chunks as they came off
 * the disk; table: [n][5] int64 device, one row { src_off, src_len, dst_off, dst_len, raw } per block: the block's bytes in src, where
 * its decoded bytes belong in dst (dst_bytes of device memory, 16-byte aligned, not overlapping src: the `staged` of
 * yogo_zarr_unpack), and whether they are copied (raw != 0, src_len == dst_len) or one LZ4 block.  One wavefront per row.
 * status: [n] int32 device, per row 0 or the check that ended it: 1 a literal run passes the end of the source, 2 the source ends
 * inside a sequence, 3 a match offset of 0 or beyond what the block has produced, 4 a copy would pass dst_len, 5 the block ends
 * before dst_len, 6 the row does not lie inside src / dst.  No byte outside a row's two ranges is read or written, whatever
 * the stored bytes say (the same checks, in the same order: yogo_amd.blosc.lz4_block_status). */
int yogo_blosc_lz4_decode(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                          long long dst_bytes, int* status, yogo_stream_t stream);
/* Zstandard frames decoded on the device in front of yogo_zarr_unpack: the blocks of Blosc chunks whose inner codec is zstd (one frame
 * per block; yogo_amd/blosc.py parses the chunk headers) and the chunks of zarr's `zstd` codec (one frame per chunk); launched from
 * yogo_amd/device_decode.py.  src, table, dst and status as yogo_blosc_lz4_decode takes them: rows { src_off, src_len, dst_off, dst_len,
 * raw }, raw != 0 copied (src_len == dst_len), else ONE frame that decodes to exactly dst_len bytes.  work: work_bytes of device memory,
 * 16-byte aligned, overlapping neither src nor dst, at least yogo_zstd_work_bytes(n) (128 KB per row: a block's Huffman-coded
 * literals).  One wavefront per row; raw, RLE and compressed blocks; raw, RLE, Huffman-compressed (1 or 4 streams, direct or
 * FSE-compressed weights) and treeless literals; predefined, RLE, FSE-compressed and repeated tables; repeat offsets; offset codes up
 * to 31.  The window size is parsed and not enforced (a match may reach back over all the frame has produced); a content checksum must
 * be present when flagged and is NOT verified.  status: [n] int32 device, per row 0 or the check that ended it: 1 the row does not
 * lie inside src / dst / work, 2 the source or a block ends inside a header or a section, 3 no frame magic (a skippable frame too),
 * 4 a reserved bit or a dictionary id in the frame header, 5 the frame content size is not dst_len, 6 block type 3 or a block above
 * 128 KB, 7 an invalid literals section (above 128 KB, stream sizes past the section, treeless without a table), 8 Huffman weights that
 * describe no code of at most 11 bits, 9 an invalid FSE table (accuracy log or symbol above the limit, counts that do not sum up,
 * repeat mode without a table), 10 a backward bitstream that is empty, lacks its marker bit or is not consumed exactly, 11 an invalid
 * sequences section (reserved mode bits, bytes after zero sequences, a literal length past the block's literals), 12 a match offset
 * of 0 or beyond what the frame has produced, 13 the frame would pass dst_len, 14 it ends before dst_len, 15 bytes after the frame's
 * end.  No byte outside a row's ranges is read or written, whatever the stored bytes say (the same checks, in the same order:
 * yogo_amd.zstd.zstd_frame_status). */
int yogo_zstd_work_bytes(int n, size_t* bytes);
int yogo_zstd_decode(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                     long long dst_bytes, int* status, unsigned char* work, long long work_bytes, yogo_stream_t stream);
/* The chunks of a zarr stack under the `zlib` codec, inflated on the device in front of yogo_zarr_unpack (yogo_amd/inflate.py takes
 * the zlib wrapper off on the host: split_zlib).  src: src_bytes of device memory holding stored chunks as they came off the disk;
 * table: [n][5] int64 device, one row { src_off, src_len, dst_off, dst_len, adler32 } per stream: its raw DEFLATE bytes in src
 * (between the 2-byte header and the 4-byte trailer), where exactly dst_len inflated bytes belong in dst (dst_bytes of device
 * memory, 16-byte aligned, not overlapping src), and the trailer's Adler-32.  One wavefront per row; stored, fixed and dynamic
 * blocks, code-length sets held to zlib's rule.  status: [n] int32 device, per row 0 or the check that ended it: 1 the row does not
 * lie inside src / dst, 2 block type 3, 3 a stored block's LEN / NLEN do not match, 4 the source ends inside a token, 5 invalid
 * code lengths in a dynamic header, 6 a code or symbol the format does not define (a pattern without a code, literal / length
 * symbol 286 / 287, distance code 30 / 31), 7 a distance beyond what the stream has produced, 8 the stream would pass dst_len,
 * 9 it ends before dst_len, 10 dst_len bytes came out and their Adler-32 is not the trailer's.  No byte outside a row's two
 * ranges is read or written, whatever the stored bytes say (the same checks, in the same order: yogo_amd.inflate.inflate_status). */
int yogo_inflate_zlib(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                      long long dst_bytes, int* status, yogo_stream_t stream);
/* Baseline JPEG files decoded on the device to the planes `read_image` gives (PIL on libjpeg's defaults: JDCT_ISLOW, fancy
 * upsampling), in front of the PNG unpack kernels, which take them as planar entries (yogo_amd/png_batch.py; `--device-image-decode-jpeg`).
 * src: src_bytes of device memory holding the files as they came off the disk, at any alignment; table: [n][18] int64 device, one row
 * { src_off, src_len, dst_off, dst_len, H, W, components | luma h << 8 | luma v << 16, restart interval, scan_off, quant[3], dc[3],
 * ac[3] } per file (yogo_amd.jpeg.table_row): the file's bytes in src; where its C_out * H * W == dst_len output bytes belong in dst
 * (dst_bytes of device memory, not overlapping src): [C_out][H][W] uint8, C_out 1 (grey; from colour PIL's luma of R, G, B) or 3 (R, G,
 * B; from grey the plane three times); the frame; where the entropy-coded bytes start; per component 2 * the offset of its 64
 * quantiser entries + (1: 16-bit entries) and the offsets of the 16 counts of its DC and AC Huffman tables, from the file's first byte,
 * -1 for a table never defined.  The kernel reads DQT / DHT from the file at these offsets (no descriptor is uploaded) and trusts
 * none of them.  Served: SOF0 / SOF1, 8 bits, one interleaved scan, grey or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, restart intervals, W <=
 * 1040 (the LDS band: one MCU row of coefficients).  One wavefront per file; two launches, the grey rows and the colour rows.
 * status: [n] int32 device, per row 0 (every MCU decoded, the scan consumed exactly, EOI behind it) or the check that ended it:
 * 1 the row does not lie inside src / dst or describes no frame the kernel takes, 2 a table the scan names was never defined or does
 * not lie inside the file, 3 a DHT whose counts describe no prefix code (or use the all-ones code) or more than 256 symbols, 4 the
 * source ends inside a code, inside extra bits or in front of a restart marker, 5 a bit pattern without a code, 6 a DC category
 * above 11, an AC category above 10 or an AC symbol r/0 with r in 1 .. 14, 7 a run that passes coefficient 63, 8 a marker inside a
 * restart interval, FF followed by neither 00 nor an allowed marker, bytes left over in front of a restart marker or another marker
 * than the expected RSTm, 9 no EOI behind the last MCU, 10 EOI in front of the last MCU, 11 a dequantised coefficient outside
 * +-2047.  Whatever libjpeg would repair with a warning is a nonzero status: the file is the host's.  A row with a nonzero status may
 * have written part of its own dst range; no byte outside a row's two ranges is read or written, whatever the stored bytes say (the
 * same checks, in the same order: yogo_amd.jpeg.jpeg_status). */
int yogo_jpeg_decode(const unsigned char* src, long long src_bytes, const long long* table, int n, unsigned char* dst,
                     long long dst_bytes, int C_out, int* status, yogo_stream_t stream);

/* ---- PNG directories for inference (yogo_amd/png_feed.py, `yogo infer --path-to-images --device-image-decode`) ---------------
 * The scanlines of 8-bit greyscale, non-interlaced PNG files as yogo_inflate_zlib leaves them (the IDAT payloads of a file are one
 * zlib stream; yogo_amd/png.py parses the chunks on the host) -> a batch: the PNG filters reversed, CenterCrop and the optional
 * / 255 in one launch.  scan: scan_bytes of device memory; table: [B][2] int64 device, one row { off, raw } per image: where it
 * lies in scan, and whether it is H scanlines of 1 + W bytes with the filter-type byte first (raw = 0) or H x W pixels as they are
 * (raw != 0: an image the host decoded).  Filter types 0 .. 4 with one byte per pixel, the row above row 0 zeros, arithmetic
 * mod 256, the Paeth predictor's ties in the order left, above, upper-left.  scan is WRITTEN: the last row of every band of 64 rows
 * is unfiltered in place (the next band reads it), the rest is left as it was.  out: [B][1][OH][OW] uint8 (out_fp32 = 0) or fp32
 * x / 255 bit-identical to torch's CPU uint8_tensor / 255 (out_fp32 = 1): out[b][0][oy][ox] = image_b[top + oy][left + ox],
 * 1 <= OH <= H - top, 1 <= OW <= W - left.  status: [B] int32 device, per image 0, 1 (a filter-type byte above 4: its rows from
 * that band on are not written) or 2 (the image does not lie inside scan: nothing of it is read).  One wavefront per image,
 * 64 rows at a time, skewed by one pixel per row (csrc/png_unfilter.h: the loop yogo_png_unpack_planes runs too; the launch wrappers
 * of both are in yogo_amd/device_decode.py).  B <= 65535, H, W <= 65535. */
int yogo_png_unpack(unsigned char* scan, long long scan_bytes, const long long* table, int B, int H, int W, int top, int left, int OH,
                    int OW, void* out, int out_fp32, int* status, yogo_stream_t stream);

/* ---- PNG files into the device image cache (yogo_amd/png_prefill.py, `yogo train --device-image-cache GIB --device-image-decode`)
 * yogo_png_unpack for full frames of 1 or 3 planes, from 8-bit greyscale AND 8-bit RGB files: same scan buffer, same [B][2] int64
 * table { off, kind }, kind 0: H scanlines of 1 + W bytes (grey); kind 2: H scanlines of 1 + 3 W bytes (RGB, the filters at 3 bytes
 * per pixel: a byte's left neighbour is the same channel of the pixel to the left); kind 1: C_out x H x W planar pixels as they
 * are (an image the host decoded).  out: [B][C_out][H][W] uint8 (any alignment: a view into the cache), C_out 1 or 3, no crop and
 * no / 255; the file's channels become the cache's as yogo_amd.yogo_dataset.read_image(path, rgb) does it: grey -> 1 plane as it
 * is, grey -> 3 planes the plane three times, RGB -> 3 planes de-interleaved, RGB -> 1 plane
 * L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  scan is WRITTEN as by yogo_png_unpack (the last row of every band of 64).
 * status: [B] int32 device, per image 0, 1 (a filter-type byte above 4: its rows from that band on are not written) or 2 (a kind
 * outside 0 .. 2, or the image does not lie inside scan: nothing of it is read).  One wavefront per image, 64 rows at a time,
 * skewed by one pixel per row, a 3-byte pixel in one register: csrc/png_unfilter.h's loop, so for kind 0 and C_out = 1 the output
 * is yogo_png_unpack's, bit for bit.  B <= 65535, H, W <= 65535. */
int yogo_png_unpack_planes(unsigned char* scan, long long scan_bytes, const long long* table, int B, int H, int W, int C_out,
                           unsigned char* out, int* status, yogo_stream_t stream);

/* ---- PNG files of every colour type, bit depth and interlace method (`--device-image-decode-all`, on both routes above) --------
 * yogo_png_unpack and yogo_png_unpack_planes in one, for whatever a PNG file may hold; the images of a launch may each be of another
 * format.  Same scan buffer; table: [B][3] int64 device, one row { off, fmt, pal } per image.  off: where it lies in scan.
 * fmt = colour type | bit depth << 8 | interlace << 16, IHDR's fields, for the pairs the PNG specification allows (0 at 1 2 4 8 16,
 * 2 at 8 16, 3 at 1 2 4 8, 4 and 6 at 8 16; interlace 0 or 1): the scanlines as the file's zlib stream inflates to, rows of one
 * filter-type byte and ceil(w * channels * depth / 8) bytes -- for Adam7 the seven reduced images one after the other, a pass
 * without pixels without scanlines.  fmt = 1: C_out x H x W planar pixels as they are (an image the host decoded; kind 1 of
 * yogo_png_unpack_planes).  pal: for colour type 3 where the image's palette lies in scan, 256 x 3 bytes R G B (a shorter PLTE
 * padded with zeros by the host), else ignored.  Filter types 0 .. 4 act on bytes, the byte to the left max(1, channels * depth / 8)
 * bytes back (1, 2, 3, 4, 6 or 8); a depth below 8 is unfiltered byte by byte and a byte then expanded into 8 / depth pixels, most
 * significant bits first, the padding bits of a row's last byte dropped.  Samples become 8-bit planes as
 * yogo_amd.yogo_dataset.read_image(path, rgb) (PIL) has them -- yogo_amd.png.decode_any is the restatement on the host: grey 1 / 2 /
 * 4 v * 255 / (2^depth - 1); grey 8 as it is; grey 16 min(v, 255) (a clip, not a shift); grey+alpha, RGB and RGBA the high byte of
 * each sample, alpha dropped; palette PLTE[index]; one plane from colour L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; three
 * planes from grey the plane three times.  out: [B][C_out][OH][OW], C_out 1 or 3, uint8 (any alignment: a view into the cache) or
 * fp32 x / 255 bit-identical to torch's CPU uint8_tensor / 255: out[b][c][oy][ox] = image_b[c][top + oy][left + ox],
 * 1 <= OH <= H - top, 1 <= OW <= W - left; with top = left = 0, OH = H, OW = W and uint8 the layout is yogo_png_unpack_planes's.
 * scan is WRITTEN as by yogo_png_unpack (the last row of every band of 64 rows, of every pass).  status: [B] int32 device, per
 * image 0, 1 (a filter-type byte above 4, in any pass: its rows from that band on are not written) or 2 (a fmt outside the list, or
 * the image or its palette does not lie inside scan: nothing of it is read).  No byte outside scan and the image's own output is
 * read or written, whatever the bytes say.  One wavefront per image: csrc/png_unfilter.h's loop once per pass, so for 8-bit grey
 * and 8-bit RGB the output is that of the two entries above, bit for bit.  B <= 65535, H, W <= 65535. */
int yogo_png_unpack_any(unsigned char* scan, long long scan_bytes, const long long* table, int B, int H, int W, int top, int left,
                        int OH, int OW, int C_out, void* out, int out_fp32, int* status, yogo_stream_t stream);

/* ---- other-size files into the device image cache (yogo_amd/png_prefill.py, `yogo train ... --device-image-resize`) ------------
 * Separable antialiased bilinear (triangle filter) resampling of planar uint8 images: torch._upsample_bilinear2d_aa with
 * align_corners = False, then round-half-even and a clamp to 0 .. 255 -- what yogo_amd.yogo_dataset.resize_image computes.
 * src: [n][C][Hs][Ws] uint8 device; dst: [N][C][Hd][Wd] uint8 device (any alignment: a view into the cache); image k goes to
 * dst[dst_index[k]].  The taps are made on the host (yogo_amd/resize.py: aa_taps), per axis start[n_out] int32 and
 * weights[n_out][K] fp32 zero-padded to K, and travel packed in one 8-byte aligned buffer
 *   int64 dst_index[n] | int32 start_y[Hd] | int32 start_x[Wd] | float wy[Hd][Ky] | float wx[Wd][Kx]
 * of which tables_host is the copy in host memory and tables_dev the same bytes in device memory.  The host copy is checked before
 * anything is launched (YOGO_ERR_ARG, nothing written): dst_index distinct and inside [0, N); per axis the starts ascending and
 * inside the source, every weight in [0, 1], none on an index past the source, each output's weights summing to 1; K <= 18 and a
 * down-scale of at most 8 per axis (any up-scale); the tables' spans within what a tile stages.  So every source index the kernel
 * forms lies in [0, n_in) and it needs no status.  Arithmetic: the horizontal pass into an fp32 intermediate, then the vertical
 * one; each sum from 0 in ascending tap order with fmaf; rintf, then the clamp.  One workgroup per (image, plane, TH x 64 output
 * tile), the source rows staged in LDS, TH sized from the tables so that several workgroups share a CU.  n, C <= 65535. */
int yogo_resize_aa_u8(const unsigned char* src, int n, int C, int Hs, int Ws, unsigned char* dst, int N, int Hd, int Wd,
                      const void* tables_host, const void* tables_dev, int Ky, int Kx, yogo_stream_t stream);

/* ---- drawn boxes and their PNG files (yogo_amd/draw.py, `yogo infer --draw-boxes --device-draw`) --------------------------------
 * yogo_draw_boxes: the RGBA frames yogo_amd.utils.utils.draw_yogo_prediction makes PIL draw, for a whole batch in one launch, pixel
 * for pixel (tests/_draw_ref.py is the same arithmetic in numpy, held to PIL).  img: [B][Cimg][H][W], Cimg 1 or 3, uint8
 * (img_fp32 = 0) or float32 (img_fp32 = 1; truncated toward zero, after one fp32 multiply by 255 when normalised = 1 -- not
 * rounded, as the host route); grey is replicated, alpha is 255.  rows: [B][cap][P] fp32 and counts: [B] int32 as
 * yogo_format_preds_batched leaves them with box_format xyxy, P = 5 + classes; image b draws rows [0, counts[b]) in order, each its
 * outline and then its label.  Corners: x = fp32(W) * row[0|2], y = fp32(H) * row[1|3] in fp32, truncated toward zero; the outline
 * one pixel wide and clipped -- rows y0 and y1 from x0 to x1, columns x0 and x1 from min(y0 + 1, y1) to max(y0 + 1, y1) -- in
 * colours[class] ([classes][4] RGBA bytes, 4-byte aligned), class the first maximum of row[5:].  The label is a mask of the glyph
 * atlas blended with black, per channel t = (255 - m) * old + 128, new = ((t >> 8) + t) >> 8, alpha left at 255, at
 * (int(x) + offset x, int(y) + offset y) of the first corner.  Atlas (yogo_amd.draw.GlyphAtlas.tables): label_meta [classes][6]
 * int32 { first x cut, x cuts, first y cut, y cuts, first variant, 0 }; cuts [n_cuts] fp32; variants [n_variants][5] int32
 * { width, height, offset x, offset y, where its width * height bytes start in glyphs }; the variant of a label is
 * first + ix * (y cuts + 1) + iy with ix / iy the number of the axis' cuts at or below the fraction of the corner's x / y (the
 * fraction carries the coordinate's sign; compared as ordered bit patterns, so denormal cuts hold).  A variant outside the tables
 * or the glyph bytes draws no text.  out: [B][H][W][4] uint8, 4-byte aligned.  One workgroup per 16 x 64 tile; the operations that
 * meet the tile are compacted in order into LDS and every lane applies them to its pixels in that order. */
int yogo_draw_boxes(const void* img, int img_fp32, int normalised, int B, int Cimg, int H, int W, const float* rows, const int* counts,
                    int cap, int P, const unsigned char* colours, const int* label_meta, const float* cuts, int n_cuts,
                    const int* variants, int n_variants, const unsigned char* glyphs, long long glyph_bytes, unsigned char* out,
                    yogo_stream_t stream);
/* yogo_png_encode: [B][H][W][bpp] uint8 pixels on the device -> B complete PNG files (8 bits per sample; bpp 1 grey, 2 grey+alpha,
 * 3 RGB, 4 RGBA; no interlace), byte for byte what yogo_amd.png_encode.encode_png_host writes, which states the choices: the filter
 * per scanline by the smallest sum of absolute signed values (ties to the lowest type), bands of 16 scanlines each one
 * dynamic-Huffman block of literals only (or stored blocks when that is not smaller) in an IDAT chunk of its own, CRC-32 and
 * Adler-32 computed on the device.  yogo_png_encode_bound (on the host): slot_bytes, which no file of that shape exceeds, and
 * work_bytes, the work space ONE image needs.  files: device memory of B * slot_bytes bytes; file b starts at b * slot_bytes
 * (packed = 0) or at offsets[b], the files one after the other (packed = 1).  offsets: [B + 1] int64 device, the running sum of
 * the files' lengths in both modes (the length of file b is offsets[b + 1] - offsets[b]).  status: [B] int32 device, 0, 1 (the file
 * is longer than slot_bytes: nothing of it is written, its length counts as 0) or 2 (a band passed its part of the work space;
 * the stored fallback bounds every band, so this is a defect).  work: work_bytes >= B * the per-image size, 16-byte aligned.  Two
 * launches (bands; assembly).  No byte outside a file's slot and the work space is written.  B <= 65535, H, W <= 65535.
 * The _level forms take the compression level: 0 is the above (what the forms without a level mean), 1 codes a band as one
 * dynamic-Huffman block of literals and LZ77 matches (candidates at the distances bpp * k, k = 1 .. 64; pieces of 512 bytes parsed
 * greedily on their own: yogo_amd/png_encode.py) and is smaller or, for a band that does not compress, the same stored blocks.
 * slot_bytes is the same at both levels; work_bytes is larger at level 1 (a band's filtered bytes and its tokens are kept there) and
 * work space sized for another level is refused.  Any other level is refused. */
int yogo_png_encode_bound(int H, int W, int bpp, size_t* slot_bytes, size_t* work_bytes);
int yogo_png_encode_bound_level(int H, int W, int bpp, int level, size_t* slot_bytes, size_t* work_bytes);
int yogo_png_encode_level(const unsigned char* pixels, int B, int H, int W, int bpp, int level, unsigned char* files, long long slot_bytes,
                          int packed, long long* offsets, int* status, unsigned char* work, long long work_bytes, yogo_stream_t stream);
int yogo_png_encode(const unsigned char* pixels, int B, int H, int W, int bpp, unsigned char* files, long long slot_bytes, int packed,
                    long long* offsets, int* status, unsigned char* work, long long work_bytes, yogo_stream_t stream);

/* ---- optimiser: torch.optim.AdamW over one flat buffer, yogo/train.py:213-217,324 ---------------------------------------- */
int yogo_adamw_step(float* p, const float* g, float* m, float* v, long long n, int step, double lr, double beta1,
                    double beta2, double eps, double weight_decay, double grad_scale, yogo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* YOGO_HIP_H */
