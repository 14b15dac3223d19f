/*
 * se3conv_fps.h -- farthest-point sampling of libse3conv_hip.so: what the reference's pc/FPSSubSample.py asks of
 * `torch_cluster.fps`, per batch element, as one capturable call with a deterministic, bit-reproducible contract (the
 * reference draws a random start and leaves everything else to torch_cluster; nothing there is normative).
 *
 * Same conventions as se3conv.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, no
 * environment variable, int status).  These entry points are additions inside SE3_ABI_VERSION 6: se3conv.h and its version
 * number are unchanged.
 *
 * Contract
 *
 * - Elements.
 *   - The present rows are the first `min(n_rows, *n_valid)` (`n_valid` NULL: all `n_rows`; the word is clamped to
 *     `[0, n_rows]`).  Nothing is read from a row behind the count: not its point and not its batch id.
 *   - Element `b` is the run of present rows with `batch_ids == b`; `n_b` is its length.  An id that no row carries is an
 *     empty element with 0 samples.
 *   - `batch_ids` must be non-decreasing and inside `[0, n_batches)`.  The preparation launch checks this on the present
 *     rows; if it fails `info[2] = 1`, no sampling loop runs on the data, `info[0] = info[1] = 0`, every `out_starts` word
 *     is 0 and all `ids` are -1 (`d2_at_pick` -1.0f).
 * - Sample counts.  `m_b = min(n_b, (int)ceilf((float)n_b * ratio))` with the product rounded to fp32, as torch_cluster
 *   forms it; `0 < ratio <= 1`.  `out_starts` is the exclusive prefix sum of `m_b` (`out_starts[n_batches] = M`),
 *   `info[0] = M = sum of m_b`.
 * - Distance.  `d(i,p) = ((dx*dx) + (dy*dy)) + (dz*dz)` with `dx = x_i - x_p` and so on, in fp32, EVERY operation rounded
 *   on its own: no fused multiply-add anywhere.  This is what a few lines of numpy reproduce bit for bit.
 * - First pick.  The first pick of element `b` is its row `min(max((int)floorf(start_u[b] * n_b), 0), n_b - 1)` (fp32
 *   product; `start_u` uniform numbers in [0,1)), its first row when `start_u` is NULL.
 * - Greedy step.  `mind[i]` starts at +inf.  After each pick `p`: `mind[i] = fminf(mind[i], d(i,p))` for every row of the
 *   element, and `p` is marked.  The next pick is the UNMARKED row with the largest `mind`; ties go to the lowest row index.
 *   Hence the ids of an element are distinct, in range and listed in pick order, also on clouds with duplicate points
 *   (where `mind` is 0 for every row that is left).
 * - Outputs.  `ids[out_starts[b] + j]` is the j-th pick of element `b` as a row index of `pts` (NOT relative to the
 *   element).  `d2_at_pick[out_starts[b] + j]` (optional) is `mind` of that pick at the moment it was chosen, +inf for a
 *   first pick: non-increasing inside an element, the squared coverage radius of every prefix of the picks.
 * - Capacity.  Positions `>= capacity` are not written.  If `M > capacity`, `info[1] = 1` (else 0) and the positions below
 *   `capacity` hold exactly what the untruncated call would hold there.  `ids` and `d2_at_pick` in
 *   `[min(M, capacity), capacity)` are -1 and -1.0f.  `capacity = n_rows` can never overflow.
 * - Every byte of every output is written (`ids`, `d2_at_pick` up to `capacity`; `out_starts`; `info`), and nothing depends
 *   on what the outputs or the workspace held before the call.
 * - Non-finite coordinates.  Which rows are picked is unspecified (a NaN distance leaves `mind` as it is).  Ids stay
 *   distinct and in range, and the call neither hangs nor writes out of bounds: the iteration count is fixed by `m_b`.
 * - Errors, all decided on the host before the first launch:
 *   - a NULL `ids`, `out_starts`, `info` or `workspace`, NULL `pts` / `batch_ids` with `n_rows > 0`, `n_rows < 0`,
 *     `n_batches < 1`, `capacity < 0`, `ratio` outside `(0, 1]` (NaN included): SE3_ERR_INVALID_ARGUMENT;
 *   - `n_rows >= 2^31` or `capacity >= 2^31`: SE3_ERR_UNSUPPORTED;
 *   - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 *
 * Launches: a preparation launch of one workgroup (sortedness and range check, element boundaries by binary search in the
 * sorted ids, `m_b`, `out_starts`, `info`), the fill of the padded tails of `ids` / `d2_at_pick`, and the sampling kernel.
 *
 * Sampling kernel and its KNOWN COST.  ONE workgroup of 1024 threads per element; the loop over picks is sequential by
 * nature (pick j+1 depends on pick j).  No workgroup waits for another and nothing spins on global memory.  Elements of up
 * to SE3_FPS_RESIDENT_MAX rows keep their points and `mind` in registers for the whole loop (8 rows per thread); larger
 * ones re-read the points on every pick and keep `mind` in the workspace.  Per pick: the lanes' update and argmax, a
 * cross-lane reduction of one 64-bit key per wavefront (`mind` bits | complemented row index; marked rows have key 0), one
 * barrier (double-buffered LDS slots), the winner's coordinates read from its wavefront's slot.  With one workgroup per
 * element the machine is mostly idle on small batches (about 1.6 us per pick in the resident form: 32 x 2 200 points at
 * ratio 0.25 take 0.9 ms), and a single scene of 150 k points at ratio 0.25 takes 1.1 s on ONE compute unit (30 us per
 * pick in the streaming form): that is inherent to exact FPS without grid-wide barriers, which this library does not use.
 * Cooperative multi-workgroup elements are out of scope.  profiles/fps.txt holds the measured times.
 */
#ifndef SE3CONV_FPS_H_
#define SE3CONV_FPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* largest element (rows) the register-resident form of the sampling kernel takes: 1024 threads x 8 rows */
#define SE3_FPS_RESIDENT_MAX 8192

/* element boundaries and one fp32 word per row; 0 for invalid arguments */
size_t se3_fps_workspace_bytes(int64_t n_rows, int32_t n_batches);

int se3_fps(const float* pts,            /* [n_rows,3] */
            const int32_t* batch_ids,    /* [n_rows] non-decreasing, in [0, n_batches) */
            int64_t n_rows,
            const int32_t* n_valid,      /* device word, may be NULL = n_rows; clamped to [0, n_rows] */
            int32_t n_batches,           /* host */
            float ratio,                 /* host; 0 < ratio <= 1 */
            const float* start_u,        /* [n_batches] device, may be NULL = first row of every element */
            int64_t capacity,            /* host; rows of ids / d2_at_pick */
            int32_t* ids,                /* [capacity] */
            float* d2_at_pick,           /* [capacity], may be NULL */
            int32_t* out_starts,         /* [n_batches+1] */
            int32_t* info,               /* [3]: M, overflow flag, bad batch_ids flag */
            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_FPS_H_ */
