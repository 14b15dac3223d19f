/*
 * se3conv_seg_head.h -- the loss and metrics head of libse3conv_hip.so: the mean label-smoothed cross-entropy over the rows
 * that count, its gradient, and the per-class counters of the reference's `SemSegMetrics` (ground truth, predicted, hit), on
 * ordinary and on PADDED clouds (se3conv_padded.h), without an atomic on a float or on global memory and in a fixed order of
 * additions: two calls give the same bits, and a padded call gives the bits of the call on the trimmed arrays.  One pass over
 * the logits gives the loss and adds the counts; one pass gives the gradient.  It replaces, inside a captured step, the
 * boolean-mask compaction of the output cloud, torch's `cross_entropy` and the device-to-host copy of the logits that the
 * reference's training loops (tasks/SemSeg/train_*_rot.py, tasks/Classification/train_rot.py) make per step.
 *
 * Same conventions as se3conv_global_pool.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, int
 * status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Shapes
 * - `logits` is `[n_rows, classes]` fp32: one row per labelled row -- a point for segmentation, a batch element for
 *   classification.  Frames are already pooled.
 * - `labels` is `[n_rows]`, int32 or int64 as `label_bits` (32 or 64) says: torch labels are int64, and no conversion launch
 *   is wanted.
 * - `counted` is NULL or `[classes]` bytes, nonzero meaning that the class counts.
 * - `n_valid` is NULL (every row is present) or an int32 device word, clamped to `[0, n_rows]`: the present rows are the
 *   first `P` of them.
 * - `loss` (fp32) and `count` (int32) are one word each.
 * - `lse` is `[n_rows]` fp64, or NULL when no backward call follows.
 * - `tallies` is NULL or `[3, classes]` int64: ground truth, predicted, hit.
 * - `grad_loss` is one fp32 device word; `grad_logits` is `[n_rows, classes]` fp32.
 *
 * Which rows count
 * - A row counts iff it is present, its label lies in `[0, classes)`, and `counted` is NULL or `counted[label] != 0`.
 * - `ignore_index = -100` is therefore just an out-of-range label.
 * - No absent row of `logits` and no absent label is read.
 *
 * Arithmetic of a counted row, all in fp64 on the fp32 inputs (tests/seg_head_reference.py restates it in numpy)
 * - `m = max_c x_c`.
 * - `lse = m + log(sum_c exp(x_c - m))`, with `c` ascending.
 * - `eps = (double)smoothing`.
 * - `row = (1 - eps) * (lse - x_label) + (eps / classes) * (classes * lse - sum_c x_c)`, with `c` ascending.
 * Why fp64: a 21-class row is a few dozen transcendental calls, and the numpy restatement holds to one fp32 unit of the loss
 * without emulating a device `expf`.  What it costs is in profiles/seg_head.txt: the pass is bound by that arithmetic, not by
 * reading the logits, and at 99 000 x 21 loss, counters and gradient still take less than half the time of torch's fp32
 * `cross_entropy` forward and backward.
 *
 * The sum and its outputs
 * - Chunk `s` is rows `[s * SE3_SEG_HEAD_CHUNK, (s + 1) * SE3_SEG_HEAD_CHUNK)`: a function of the row index alone.
 * - A chunk's partial starts at `+0.0` and adds its counted rows' `row` in ascending row order.
 * - The total starts at `+0.0` and adds the partials of the chunks that hold a present row in ascending `s`.
 * - `count` is the number of counted rows.
 * - `loss = (float)(total / (double)max(count, 1))`.
 * - `lse[r]` is the row's `lse`, and `0.0` for every other row of the buffer.
 * - With no counted row, `loss = +0.0f` and `count = 0`.
 *
 * Tallies
 * - For every counted row, `pred` is the first maximum of the row: the scan starts at class 0, a later class replaces an
 *   earlier one only when `v > best`, and a NaN never replaces.
 * - Then `tallies[0][label]++`, `tallies[1][pred]++`, and `tallies[2][label]++` when `pred == label`.
 * - `tallies` is the ONE read-modify-write buffer of the library: where the other headers say "every byte is written", this
 *   call ADDS to what the buffer holds, so that an epoch accumulates on the device.  The caller zeroes it.
 * - Integer counts are exact in any order: a workgroup builds its histograms with integer LDS atomics.  No atomic touches
 *   global memory and none touches a float: partial sums, counts and histograms go through the workspace, and a finishing
 *   launch adds them.
 * - Every byte of every other output is written; nothing depends on what they, the workspace or the absent rows held.
 *
 * se3_seg_loss_bwd (`lse`, `count` as the forward call wrote them)
 * - For a counted row, `grad_logits[r, c] = (float)((double)g * (exp((double)x_c - lse_r) - q_c) / (double)max(count, 1))`
 *   with `g = *grad_loss` and `q_c = eps / classes + (c == label ? 1 - eps : 0)`.
 * - Every other row of the buffer is `0.0f`: the gradient that arrives at absent and unlabelled rows is zero by
 *   construction.
 *
 * What the order buys: two calls give the same bits; a padded call gives, on the present rows and in `loss`, `count` and
 * `tallies`, the bits of the call on the trimmed arrays.  It does not buy bit equality with numpy: `exp` and `log` are the
 * device library's, not the host's.
 *
 * Workspace: `se3_seg_head_workspace_bytes(n_rows, classes)` bytes -- per chunk one fp64 partial, one int32 count and
 * `3 * classes` int32 histogram entries; 0 for arguments the calls refuse.
 *
 * Errors, all checked on the host before the first launch
 * - a negative `n_rows`, `classes < 1`, `label_bits` not 32 or 64, `smoothing` outside `[0, 1]` or NaN, a NULL required
 *   pointer (`loss`, `count`, the workspace; `logits` and `labels` when there are rows; of the backward call `count`,
 *   `grad_loss`, and `logits`, `labels`, `lse`, `grad_logits` when there are rows): SE3_ERR_INVALID_ARGUMENT;
 * - `classes > 1024` or `n_rows * classes >= 2^31`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 * `n_rows == 0` and a word of 0 are valid.
 */
#ifndef SE3CONV_SEG_HEAD_H_
#define SE3CONV_SEG_HEAD_H_

#include <stddef.h>
#include <stdint.h>

#define SE3_SEG_HEAD_CHUNK 256   /* rows per chunk of the loss sum: part of the arithmetic contract */

/* The widest row of the LDS-tile form of the kernels: a workgroup stages its chunk's `CHUNK x classes` floats in LDS up to
 * this width and reads its rows from memory beyond it.  Not part of the arithmetic contract -- both forms compute the same
 * bits -- but the tests name a width on each side of it. */
#define SE3_SEG_HEAD_TILE_CLASSES 56

#ifdef __cplusplus
extern "C" {
#endif

/* host only */
size_t se3_seg_head_workspace_bytes(int64_t n_rows, int32_t classes);

int se3_seg_loss_fwd(const float* logits, const void* labels, int32_t label_bits, const uint8_t* counted, int64_t n_rows,
                     const int32_t* n_valid, int32_t classes, float smoothing, float* loss, int32_t* count, double* lse,
                     int64_t* tallies, void* workspace, size_t workspace_bytes, void* stream);

int se3_seg_loss_bwd(const float* logits, const void* labels, int32_t label_bits, const uint8_t* counted, const double* lse,
                     const int32_t* count, const float* grad_loss, int64_t n_rows, const int32_t* n_valid, int32_t classes,
                     float smoothing, float* grad_logits, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_SEG_HEAD_H_ */
