/*
 * se3conv_levels.h -- a chain of grid sub-sampling levels of libse3conv_hip.so in ONE call, every level written into a
 * buffer of the caller's size and the level sizes kept in device words: the hierarchy build (pc/PointHierarchy.py:40-51,
 * pc/GridSubSample.py:43-93) without a host synchronisation, capturable into a HIP graph and replayable on a batch with
 * another point count.
 *
 * Same conventions as se3conv.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, int status).
 * These entry points are additions inside SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Contract
 *
 * Level l reads `n_in` rows: `n_rows` for level 0, `capacity` of level l-1 otherwise (level l+1 reads the `pts` and
 * `batch_ids` outputs of level l in place).
 *
 * - Present and absent rows.
 *   - Level 0's present rows are `[0, *n_valid)` (`n_valid` NULL: all `n_rows`; the word is clamped to `[0, n_rows]`).
 *   - Level l's present rows are `[0, min(info[l-1][0], capacity of level l-1))`.
 *   - Nothing is read from an absent row: not its point and not its batch id.
 * - Per level. On the present rows alone the result is what `se3_grid_subsample` (se3conv.h) computes on an array that
 *   holds only those rows, bit for bit; with `u` it is additionally what `se3_grid_pick` and two row gathers compute.
 *   - Boxes widened by 1e-6, cell counts and 64-bit keys as there.
 *   - Cells are numbered in ascending key order; inside a cell the rows keep their input order.
 *   - A cell's point is the in-order sum of its rows divided once (`__fdiv_rn`); its batch id is that of its first row.
 *   - `sorted_ids` is a permutation of `[0, n_in)`: present rows grouped by cell, then the absent rows, ascending.
 * - Every byte of every output is written.
 *   - `count = min(true cell count, capacity)`.
 *   - Rows `[count, capacity)` of `pts` are 0.0f; of `batch_ids`, `ids` and `picked` they are -1.
 *   - `cell_ends[j]` is the number of present input rows for `j >= count`.
 *   - `cell_ids` of an absent row is -1.
 *   - Nothing depends on what the outputs or the workspace held before the call.
 * - Overflow (true cell count > capacity).
 *   - `info[l] = (true cell count, 1)`; without overflow `(true cell count, 0)`.
 *   - The `capacity` cells with the smallest keys are kept.  Rows of dropped cells get `cell_ids = -1`; they stay in
 *     `sorted_ids`, behind the rows of the kept cells.
 *   - Deeper levels are built from the truncated level, consistently: `info[l'][0]` for `l' > l` counts the truncated
 *     hierarchy, and only the FIRST flagged level's count is the size to run again with.
 *   - Nothing is written outside a buffer's stated extent in any case.
 * - `capacity = n_in` can never overflow (cells <= rows): outputs sized by the input count.
 * - Empty input (`n_rows == 0` or `*n_valid == 0`): every count is 0 and every pad is written.
 * - Errors, all checked on the host before the first launch:
 *   - `n_rows >= 2^31/3` or a `capacity >= 2^31/3`: SE3_ERR_UNSUPPORTED;
 *   - `n_rows < 0`, `n_batches < 1`, `n_levels < 1`, `cell_size <= 0`, `capacity < 1`, a NULL `levels`, `info` or
 *     `workspace`, NULL `pts` / `batch_ids` with `n_rows > 0`, a NULL required pointer of a level (`cell_ids` and
 *     `sorted_ids` of level 0 may be NULL when `n_rows == 0`), `u`, `ids` and `picked` neither all NULL nor all given:
 *     SE3_ERR_INVALID_ARGUMENT;
 *   - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 *
 * What reads the padded levels afterwards -- per-batch boxes, ball query, self-k-NN and PCA frames with the same kind of
 * device-side row count -- is declared in se3conv_padded.h.
 *
 * Launches per level: those of se3_grid_subsample for a level of cell averages; for a random level the pick, which also
 * gathers the level's points and batch ids, replaces the average and the batch-id kernel (one launch fewer).
 */
#ifndef SE3CONV_LEVELS_H_
#define SE3CONV_LEVELS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct se3_level {
  float    cell_size;        /* host; > 0 */
  int64_t  capacity;         /* host; rows of this level's outputs, >= 1 */
  /* maps from this level's INPUT rows (n_in = n_rows for level 0, capacity of level l-1 otherwise) */
  int32_t* cell_ids;         /* [n_in]      cell of every input row, cells numbered in ascending key order; -1 = absent row or dropped cell */
  int32_t* sorted_ids;       /* [n_in]      a permutation of [0, n_in): present rows grouped by cell (input order inside a cell), absent rows last, ascending */
  int32_t* cell_ends;        /* [capacity]  inclusive end offsets into sorted_ids */
  /* the level itself */
  float*   pts;              /* [capacity,3] */
  int32_t* batch_ids;        /* [capacity]   */
  /* random one-point-per-cell form (GridSubSample(..., p_rnd_sample=True)); all three NULL = cell averages */
  const float* u;            /* [capacity] uniform draws in [0,1), one per cell in ascending key order */
  int32_t* ids;              /* [capacity] start(c) + min(floor(u[c]*count(c)), count(c)-1): se3_grid_pick's rule */
  int32_t* picked;           /* [capacity] sorted_ids[ids[c]]; pts / batch_ids of the level are then those of the picked row */
} se3_level;

/* one region sized for the largest n_in of the chain, reused level after level */
size_t se3_grid_levels_workspace_bytes(int64_t n_rows, int32_t n_batches, const se3_level* levels /*host*/, int32_t n_levels);

int se3_grid_levels(const float* pts, const int32_t* batch_ids, int64_t n_rows,
                    const int32_t* n_valid,      /* device word, may be NULL = n_rows; clamped to [0, n_rows] */
                    int32_t n_batches,           /* host */
                    const se3_level* levels /*host array*/, int32_t n_levels,
                    int32_t* info,               /* [n_levels,2] device: true cell count, overflow flag */
                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_LEVELS_H_ */
