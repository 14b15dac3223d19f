/*
 * se3conv_global_pool.h -- global pooling of libse3conv_hip.so: one row per batch element out of the feature rows of a
 * cloud (the head of a classification network: `Pointcloud.global_pooling`, `global_upsample`,
 * `global_pooling_specific_feature_pooling`), on ordinary and on PADDED clouds (se3conv_padded.h), without an atomic and
 * with a fixed order of additions: two calls give the same bits, and a padded call gives the bits of the call on the
 * trimmed arrays.  With it the step of a classification network is one captured HIP graph that follows the row-count word.
 *
 * Same conventions as se3conv_padded_rows.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls,
 * int status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.  `mode` is SE3_POOL_AVG / MAX / MIN / SUM of se3conv.h.
 *
 * Shapes and the row-count word
 * - `x` is `[n_rows * frames, channels]`, row = point * frames + frame.
 * - `batch_ids` is `[n_rows]`: one id per POINT, in any order (they need not be sorted).
 * - `n_valid` is NULL (every point is present) or an int32 device word, clamped to `[0, n_rows]`: the present points are
 *   the first `P` of them.  No absent row of `x` and no absent id is read.
 * - A present point whose id lies outside `[0, n_batches)` belongs to no element: the pool skips it, the un-pooling writes
 *   a zero row for it.
 * - Every byte of every output is written; nothing depends on what the outputs, the workspace or the absent rows held
 *   before the call.
 *
 * se3_global_pool: `out [n_batches, channels]`, `arg [n_batches, channels]`, `counts [n_batches]`
 * - `counts[b]` is the number of present points of element `b`.
 * - An element without a point gets `out = +0.0f`, `arg = -1`, `counts = 0`.
 * - sum / avg.  Chunk `s` covers the points `[s * SE3_GLOBAL_POOL_CHUNK, (s + 1) * SE3_GLOBAL_POOL_CHUNK)`: a function of
 *   the row index alone, never of `n_rows` or of the word.  The partial sum of `(s, b, c)` starts at `+0.0` and adds, as
 *   fp64 and in ascending row order, `x[row, c]` of the present rows of element `b` in chunk `s`.  The total of `(b, c)`
 *   starts at `+0.0` and adds the partial sums in ascending `s`.  A partial sum is never `-0.0`, so an empty chunk is an
 *   exact identity, and the padded call equals the call on the trimmed arrays bit for bit.
 *   sum: `out = (float)total`.  avg: `out = (float)(total / (double)(counts[b] * frames))`.
 *   `arg` may be NULL; when it is not, it is filled with `-1`.
 * - max / min.  The first present row of the element seeds the result; a later row replaces it when `v > best` (max) or
 *   `v < best` (min): ties go to the lowest row, and a NaN never replaces and is never replaced.  `arg[b, c]` is the row's
 *   index in `[0, n_rows * frames)`.  (Evaluated per chunk and combined by the same rule in ascending chunk order, which is
 *   the same thing.)  `arg` is required.
 * - `n_rows == 0` and `P == 0` are valid: zeros, `-1` and `0`.
 * - Workspace: `se3_global_pool_workspace_bytes(n_rows, frames, n_batches, channels)` bytes -- 8 bytes per
 *   (chunk, element, channel) and 4 per (chunk, element); 0 for arguments the call refuses.
 *
 * se3_global_unpool: `out [n_rows * frames, channels]` from `vals [n_batches, channels]` -- the gradient of the pool, and in
 * sum mode the up-sampling `vals[batch_ids[point]]` itself
 * - sum: `out[row, c] = vals[b, c]`, `b` the id of the row's point.
 * - avg: `__fdiv_rn(vals[b, c], (float)(counts[b] * frames))`.
 * - max / min: `vals[b, c]` where `arg[b, c] == row`, else `0.0f`.
 * - Absent rows, and rows of points whose id is out of range, are `0.0f`.
 * - `arg` is read by max / min only, `counts` by avg only; each may be NULL otherwise.
 *
 * Errors, all checked on the host before the first launch
 * - a negative `n_rows`, `frames < 1`, `n_batches < 1`, `channels < 1`, a mode outside 0..3, a NULL required pointer
 *   (`out`, `counts` of the pool, the workspace; `x` / `vals` and `batch_ids` when there are rows; `arg` for max / min;
 *   `counts` of the un-pooling for avg): SE3_ERR_INVALID_ARGUMENT;
 * - `n_rows * frames * channels >= 2^31` or `n_batches * channels >= 2^31`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_GLOBAL_POOL_H_
#define SE3CONV_GLOBAL_POOL_H_

#include <stddef.h>
#include <stdint.h>

/* points per chunk of the sum / avg order above: a power of two.  Part of the arithmetic contract -- a library built with
 * another value gives other last bits (tests/global_pool_reference.py holds the same number).  It trades the serial chain
 * of one (chunk, element, channel) against the size of the partial table; 128 is the measured choice among 32 .. 1024
 * (profiles/global_pool.txt). */
#define SE3_GLOBAL_POOL_CHUNK 128

#ifdef __cplusplus
extern "C" {
#endif

/* host only */
size_t se3_global_pool_workspace_bytes(int64_t n_rows, int32_t frames, int32_t n_batches, int32_t channels);

int se3_global_pool(const float* x, const int32_t* batch_ids, int64_t n_rows, int32_t frames, const int32_t* n_valid,
                    int32_t n_batches, int32_t channels, int32_t mode, float* out, int32_t* arg, int32_t* counts,
                    void* workspace, size_t workspace_bytes, void* stream);

int se3_global_unpool(const float* vals, const int32_t* batch_ids, const int32_t* arg, const int32_t* counts,
                      int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t n_batches, int32_t channels,
                      int32_t mode, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_GLOBAL_POOL_H_ */
