/*
 * se3conv_padded.h -- the geometry builds of libse3conv_hip.so on PADDED clouds: a cloud whose buffers have `n_rows` rows of
 * which only the first `*n_valid` exist, the count being a device word.  Per-batch boxes, the ball query, the self-k-NN and
 * the PCA frames of such a cloud without a host synchronisation -- what the levels of se3_grid_levels (se3conv_levels.h)
 * are handed to, so that hierarchy, frames, neighbourhoods and convolutions of a step are one captured HIP graph, replayable
 * on a batch with another point count.
 *
 * Same conventions as se3conv_levels.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls,
 * int status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Contract, common to all entry points
 *
 * A cloud argument is `(pts, batch_ids, n_rows, n_valid)`.
 *
 * - `n_valid` is an int32 device word.  NULL means `n_rows`; otherwise the word is clamped to `[0, n_rows]`.
 * - Present rows are `[0, *n_valid)`.  Their batch ids are sorted and lie in `[0, n_batches)`.
 * - Nothing is read from an absent row: not its point, not its batch id, not its k-NN row.
 * - Every byte of every output is written (the one stated exception: rows `[E, capacity)` of the ball query's lists).
 * - Nothing depends on what the outputs, the workspace or the absent rows held before the call.
 * - With `n_valid` NULL or equal to `n_rows`, a call's outputs equal those of its counterpart in se3conv.h bit for bit.
 *
 * se3_batch_aabb_padded
 * - `se3_batch_aabb` over the present rows alone.
 * - A batch element without a present row gets `(+inf, -inf)`, as an empty element gets from `se3_batch_aabb`.
 *
 * se3_ball_query_padded
 * - `se3_ball_query_bounded_shared` with a count word per cloud, `n_valid_src` and `n_valid_dst`.
 * - `grid` may be NULL: nothing is shared and the source cloud's grid is built inside the workspace.
 * - Per present sample: the same SET of sources that `se3_ball_query_bounded` finds on arrays that hold only the present
 *   rows.
 * - The order inside a sample is deterministic and does not depend on what the absent rows hold.
 *   - It need not be the order of the call on the trimmed arrays: whether every source is tested (ascending source id) or
 *     the cell grid is walked (cell order) is decided on the host, from `n_rows_src`.
 * - An absent sample has no edges: its `ends` entry equals that of the sample in front of it, and behind the last present
 *   sample every entry is the edge total.
 * - No absent source is ever listed.
 * - `info = (true edge count, overflow flag)`, the truncation on overflow (`ends` clamped to `capacity`, the head of the
 *   list kept), the optional `sources` and "rows `[E, capacity)` of `neighbors` / `sources` untouched" are those of
 *   `se3_ball_query_bounded`.
 * - `aabb_min` / `num_cells` (needed when `se3_ball_query_needs_grid(n_rows_src)`) are those of
 *   `se3_ball_query_grid_from_box` on the boxes of `se3_batch_aabb_padded`.
 * - A cloud against itself (the same `pts`, `batch_ids` and `n_valid` pointers on both sides) walks its samples in cell
 *   order; the result is the same.
 * - A shared grid (`grid_valid != 0`) built by a padded call is valid only for padded calls with the same `pts_src`,
 *   `batch_src`, `n_rows_src`, grid parameters, radius, `n_batches` and the same VALUE of the `n_valid_src` word.  The
 *   other ball queries must not be handed it.
 * - Empty input (`n_rows_dst == 0`): `info = (0, 0)`.
 *
 * se3_knn_grid_params_padded
 * - `se3_knn_grid_params` with the per-batch point counts taken over the present rows.
 *
 * se3_knn_query_padded
 * - Self-k-NN inside a padded cloud, `k <= 64`.
 * - `aabb_min`, `num_cells` and `cell_size` all given (from `se3_knn_grid_params_padded`): the cell-grid search of
 *   `se3_knn_query_grid`, `k <= 32`, workspace of `se3_knn_query_padded_workspace_bytes(n_rows, 1)`.  All three NULL: the
 *   all-pairs search of `se3_knn_query`, which needs no workspace (`workspace` may be NULL).
 * - Present rows: what `se3_knn_query` / `se3_knn_query_grid` compute on the present rows alone, bit for bit (ascending
 *   (distance, index), the point itself first, -1 where the batch element has fewer than k points).
 * - Absent rows: -1 in every column.
 *
 * se3_pca_frames_padded
 * - Present rows: the frames of `se3_pca_frames`, bit for bit.  `knn` is the output of `se3_knn_query_padded`.
 * - Absent rows: the identity in every one of the 4 (fixed axis: 2) frame copies, so that `se3_shuffle_frames`, which is
 *   row-wise, leaves identities there.
 *
 * Errors, all checked on the host before the first launch
 * - a negative row count or capacity, `n_batches < 1`, `radius <= 0`, `k < 1`, `axis_fixed > 2`, a NULL required pointer
 *   (`info`, `ends`, a workspace that is needed, the clouds when they have rows, `neighbors` with `capacity > 0`, grid
 *   parameters on the grid path, grid parameters of the k-NN neither all NULL nor all given), `capacity >= 2^31` (as in
 *   `se3_ball_query_bounded`): SE3_ERR_INVALID_ARGUMENT;
 * - `n_rows_src >= 2^31`, `n_rows_dst >= 2^31/9`, k-NN and frames `n_rows >= 2^31`, `k > 64`, `k > 32` on the cell-grid
 *   search, `axis_fixed == 0`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` (or `grid_bytes` of a grid that is given) below the query's value: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_PADDED_H_
#define SE3CONV_PADDED_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int se3_batch_aabb_padded(const float* pts, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid,
                          int32_t n_batches, float* aabb_min /*[n_batches,3]*/, float* aabb_max /*[n_batches,3]*/,
                          void* stream);

/* the value of se3_ball_query_workspace_bytes for the row counts */
size_t se3_ball_query_padded_workspace_bytes(int64_t n_rows_src, int64_t n_rows_dst);

int se3_ball_query_padded(const float* pts_src, const float* pts_dst, const int32_t* batch_src, const int32_t* batch_dst,
                          const float* aabb_min, const int32_t* num_cells, float radius, int64_t n_rows_src,
                          int64_t n_rows_dst, const int32_t* n_valid_src, const int32_t* n_valid_dst, int32_t n_batches,
                          void* grid /*may be NULL*/, size_t grid_bytes /*se3_ball_query_grid_bytes(n_rows_src)*/,
                          int32_t grid_valid, void* workspace, size_t workspace_bytes, int64_t capacity,
                          int32_t* neighbors /*[capacity,2]*/, int32_t* sources /*[capacity], may be NULL*/,
                          int32_t* ends /*[n_rows_dst]*/, int32_t* info /*[2]*/, void* stream);

int se3_knn_grid_params_padded(const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid, const float* box_min,
                               const float* box_max, int32_t n_batches, int32_t k, float cell_factor, float* aabb_min,
                               int32_t* num_cells /*[3]*/, float* cell_size /*[3]*/, void* stream);

/* use_grid != 0: the cell-grid search (se3_knn_query_grid_workspace_bytes(n_rows)); 0: the all-pairs search, 0 bytes */
size_t se3_knn_query_padded_workspace_bytes(int64_t n_rows, int32_t use_grid);

int se3_knn_query_padded(const float* pts, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid,
                         const float* aabb_min, const int32_t* num_cells, const float* cell_size, /* all NULL = all pairs */
                         int32_t k, int32_t* out /*[n_rows,k]*/, void* workspace, size_t workspace_bytes, void* stream);

int se3_pca_frames_padded(const float* pts, const int32_t* knn /*[n_rows,k]*/, int64_t n_rows, const int32_t* n_valid,
                          int32_t k, int32_t axis_fixed /* -1, 1 or 2 */, float* frames /*[n_rows, 4 or 2, 9]*/,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_PADDED_H_ */
