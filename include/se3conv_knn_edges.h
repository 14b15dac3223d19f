/*
 * se3conv_knn_edges.h -- capacity-bounded k-NN neighbourhoods of libse3conv_hip.so: the k-NN pair query between two PADDED
 * clouds (se3conv_padded.h: buffers of `n_rows` rows of which the first `*n_valid` exist, the count being a device word), and
 * the pass that turns an `[n_rows, k]` id table with -1 padding into the `(neighbors, ends, info)` triple that the
 * convolution and se3_csr_transpose_bounded consume -- without the host ever knowing the edge count.  With both, a k-NN
 * neighbourhood (a cloud against itself: se3_knn_query_padded writes the table) is built inside a captured HIP graph and
 * follows the row-count words on replay.
 *
 * Same conventions as se3conv_padded.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls,
 * int status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * se3_knn_query_pair_padded
 * - `se3_knn_query_pair` (the all-pairs search inside the batch element) with a count word per cloud, `n_valid_src` and
 *   `n_valid_q`: int32 device words, NULL = every row, otherwise clamped to `[0, n_rows]`.
 * - Present rows of a cloud are `[0, *n_valid)`; their batch ids are sorted.  Nothing is read from an absent row of
 *   either cloud: not its point, not its batch id.
 * - Present query rows: what `se3_knn_query_pair` computes on the arrays that hold only the present rows, bit for bit --
 *   ascending (fp32 squared distance, source index), -1 where the batch element has fewer than k present sources.
 * - Absent query rows: -1 in every column.
 * - Every byte of `out` is written; nothing depends on what `out` or the absent rows held before the call.
 * - `*n_valid_src == 0` (or `n_rows_src == 0`): every entry is -1.
 * - `k <= 64`.
 *
 * se3_knn_edges_bounded
 * - `ids [n_rows, k]` is a table as se3_knn_query, se3_knn_query_padded, se3_knn_query_pair or
 *   se3_knn_query_pair_padded write it: in every row the valid (non-negative) entries are a prefix.  What stands behind the
 *   first negative entry of a row is not looked at.  `n_valid` (int32 device word, NULL = every row, clamped to
 *   `[0, n_rows]`): rows from it on are absent and are not read.
 * - The edge list is sample-major: row r contributes `(r, ids[r, j])` -- column 0 the sample, column 1 the source -- for
 *   the j of its valid prefix, in table order.  `ends[r]` is the inclusive end offset of row r's group.
 * - An absent row has no edges: its `ends` entry equals that of the row in front of it, and behind the last present row
 *   every entry is the edge total.
 * - `info = (true edge count E, overflow flag)`; the flag is 1 when `E > capacity`.  On overflow the head of the list (its
 *   first `capacity` rows) is kept and `ends` is clamped to `capacity`.
 * - Every byte of `ends` and `info` is written.  Rows `[E, capacity)` of `neighbors` stay untouched: the one stated
 *   exception.  In all of this the triple is that of `se3_ball_query_bounded`.
 * - `n_rows == 0`: `info = (0, 0)`.
 * - The offsets come from a prefix sum and there are no atomics: the list is a pure function of the table and the word.
 * - `n_rows * k` is the capacity that can never overflow.
 * - Workspace: `se3_knn_edges_workspace_bytes(n_rows)` bytes; nothing depends on what it held before the call.
 *
 * Errors, all checked on the host before the first launch
 * - a negative row count or capacity, `k < 1`, a NULL required pointer (`out` / `ends` / `ids` / the query cloud / the
 *   workspace when there are rows, the source cloud when it has rows, `info`, `neighbors` with `capacity > 0`),
 *   `capacity >= 2^31`: SE3_ERR_INVALID_ARGUMENT;
 * - a row count `>= 2^31`, `n_rows * k >= 2^31`, `k > 64`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_KNN_EDGES_H_
#define SE3CONV_KNN_EDGES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int se3_knn_query_pair_padded(const float* src_pts, const int32_t* src_batch, int64_t n_rows_src, const int32_t* n_valid_src,
                              const float* q_pts, const int32_t* q_batch, int64_t n_rows_q, const int32_t* n_valid_q,
                              int32_t k, int32_t* out /*[n_rows_q,k]*/, void* stream);

/* host only */
size_t se3_knn_edges_workspace_bytes(int64_t n_rows);

int se3_knn_edges_bounded(const int32_t* ids /*[n_rows,k]*/, int64_t n_rows, const int32_t* n_valid, int32_t k,
                          int64_t capacity, int32_t* neighbors /*[capacity,2]*/, int32_t* ends /*[n_rows]*/,
                          int32_t* info /*[2]*/, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_KNN_EDGES_H_ */
