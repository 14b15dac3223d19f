/*
 * se3conv_padded_rows.h -- the row-wise passes of a network on PADDED clouds (se3conv_padded.h): batch norm, the residual
 * connection with its drop-path gate, frame pooling, and the pooling / up-sampling between the levels of se3_grid_levels
 * (se3conv_levels.h) on feature tensors that are padded like the points they belong to.  With these, everything between the
 * convolutions of a network follows the row-count words too, and one whole training step -- geometry, convolutions, glue,
 * loss and backward -- is one captured HIP graph, replayable on a batch with another point count.
 *
 * Same conventions as se3conv_padded.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls,
 * int status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Contract, common to all entry points
 *
 * A feature tensor on a padded cloud has `n_rows * frames` rows of `c` floats, row = point * frames + frame.
 *
 * - `n_valid` is an int32 device word.  NULL means `n_rows`; otherwise the word is clamped to `[0, n_rows]`.
 * - Present rows are the first `P = clamp(*n_valid, 0, n_rows) * frames`.
 * - Nothing is read from an absent row of any input: not a feature row, not a gradient row, not a `row_batch` entry.
 * - Every byte of every output is written.  Absent rows of every row-shaped output are `0.0f`; absent rows of `arg`
 *   are `-1`.
 * - Nothing depends on what the outputs, the workspace or the absent rows held before the call.
 * - Per-channel outputs (`save_mean`, `save_invstd`, `dgamma`, `dbeta`, the running statistics, `num_batches_tracked`) and
 *   the present rows of row outputs equal, bit for bit, what the counterpart in se3conv.h computes on arrays that hold
 *   only the first `P` rows, `P == 0` included.
 *   - The fp64 channel sums therefore split the rows over partial sums as the call on `P` rows would: the launched grid
 *     is sized from `n_rows * frames`, the stride and the number of live partial sums come from the word through the same
 *     integer formula on the device, and the surplus blocks contribute exact zeros.
 * - With `n_valid` NULL or equal to `n_rows`, the whole output equals that of the counterpart in se3conv.h.
 * - Workspaces are `se3_glue_workspace_bytes(c)`, as for the counterparts.
 *
 * se3_bn_fwd_padded / se3_bn_bwd_padded
 * - `se3_bn_fwd` / `se3_bn_bwd`: all statistics, the running statistics' unbiased variance and the gradient's `1/N` run
 *   over the `P` present rows.
 *
 * se3_skip_fwd_padded / se3_skip_bwd_padded
 * - `se3_skip_fwd` / `se3_skip_bwd` (`out = x * gamma * gate + y` and its gradient) with both `gate_keep` conventions.
 * - `row_batch [n_rows * frames]` of an absent row is never read.
 * - `dx` may be NULL (then `dgamma` alone is computed); `dy = g` stays "no kernel".
 *
 * se3_channel_sums_padded
 * - `sums[c] = sum over the present rows of x[r, c]`, accumulated in fp64 in the fixed order of the batch-norm statistics:
 *   the bias gradient of a point-wise linear layer inside a captured step (a framework's multi-block column sum zeroes its
 *   semaphores with a memset node).  It has no counterpart in se3conv.h; on the first `P` rows alone, with `n_valid` NULL, it
 *   gives the same bits.
 *
 * se3_frame_pool_padded / se3_frame_unpool_padded
 * - `se3_frame_pool` / `se3_frame_unpool`, all four modes; absent points get `0` (`arg`: `-1`), absent rows of `grad_x`
 *   get `0`.
 *
 * se3_segment_unpool_padded
 * - `se3_segment_unpool` where a row with `cell_ids[row] < 0` -- an absent row or a row of a dropped cell, as
 *   `se3_grid_levels` writes them -- reads nothing and gets zeros.  It takes no word: the cell ids say which rows exist.
 * - No padded form of `se3_segment_pool` is needed: called with `n_cells = capacity` on a level of `se3_grid_levels`,
 *   whose `cell_ends[j]` for `j >= count` is the number of present rows, it finds empty segments behind the kept cells,
 *   writes `0` / `arg = -1` there and reads only rows that kept segments list.
 *
 * se3_rows_gather_padded
 * - `se3_rows_gather` where `idx[r] < 0` gives a zero row (pooling through the `picked` of a random level).
 *
 * se3_rows_unpick_padded
 * - The up-sampling of a random level and the gradient of that gather, written as a gather so that nothing needs a
 *   zero-fill: `out[r] = src[cell_ids[r]]` when `cell_ids[r] >= 0` and `picked[cell_ids[r]] == r`, a zero row otherwise.
 *   `cell_ids [n_in]`, `picked [capacity]`, `src [capacity]` and `out [n_in]` rows of `row_bytes` bytes.
 *
 * Errors, all checked on the host before the first launch, with the codes of the counterparts
 * - a negative `n_rows`, `frames < 1`, a NULL required pointer, a mode outside 0..3, `row_bytes < 1`, `c < 1` or
 *   `c > 1024`: SE3_ERR_INVALID_ARGUMENT;
 * - `c > 256` with `c % 4 != 0`, or `n_rows * frames >= 2^31` (the row movers and the segment un-pooling:
 *   `n_rows >= 2^31`): SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below `se3_glue_workspace_bytes(c)`: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_PADDED_ROWS_H_
#define SE3CONV_PADDED_ROWS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int se3_bn_fwd_padded(const float* x, const float* weight, const float* bias, int64_t n_rows, int32_t frames,
                      const int32_t* n_valid, int32_t c, float eps, float momentum, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float* y, float* save_mean, float* save_invstd,
                      void* workspace, size_t workspace_bytes, void* stream);

int se3_bn_bwd_padded(const float* dy, const float* x, const float* mean, const float* invstd, const float* gamma,
                      int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t c, float* dx, float* dgamma,
                      float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

int se3_skip_fwd_padded(const float* x, const float* y, const float* gamma, const float* gate, float gate_keep,
                        const int32_t* row_batch, int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t c,
                        float* out, void* stream);

int se3_skip_bwd_padded(const float* g, const float* x, const float* gamma, const float* gate, float gate_keep,
                        const int32_t* row_batch, int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t c,
                        float* dx, float* dgamma, void* workspace, size_t workspace_bytes, void* stream);

int se3_channel_sums_padded(const float* x, int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t c, float* sums,
                            void* workspace, size_t workspace_bytes, void* stream);

int se3_frame_pool_padded(const float* x, int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t channels,
                          int32_t mode, float* out, int32_t* arg, void* stream);

int se3_frame_unpool_padded(const float* grad_out, const int32_t* arg, int64_t n_rows, int32_t frames,
                            const int32_t* n_valid, int32_t channels, int32_t mode, float* grad_x, void* stream);

int se3_segment_unpool_padded(const float* cell_vals, const int32_t* cell_ids, const int32_t* cell_ends,
                              const int32_t* arg, int64_t n_rows, int32_t channels, int32_t mode, float* out,
                              void* stream);

int se3_rows_gather_padded(const void* src, const int32_t* idx, int64_t n_out, int64_t row_bytes, void* out, void* stream);

int se3_rows_unpick_padded(const void* src, const int32_t* cell_ids, const int32_t* picked, int64_t n_in,
                           int64_t row_bytes, void* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_PADDED_ROWS_H_ */
