/*
 * se3conv_group_norm.h -- the point-cloud group norm of libse3conv_hip.so (the reference's `GroupNormPC`): every batch
 * element of a cloud normalised on its own, per group of channels, forward and backward, on ordinary and on PADDED clouds
 * (se3conv_padded.h), without an atomic and in a fixed order of additions: two calls give the same bits, and a padded call
 * gives the bits of the call on the trimmed arrays.  The statistics of an element come from its own rows alone, so a step
 * that holds one scene per GPU needs neither a second scene nor a reduction across ranks.
 *
 * Same conventions as se3conv_global_pool.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, no
 * atomics, int status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Shapes and the row-count word
 * - `x`, `dy`, `y`, `dx` are `[n_rows * frames, channels]`, row = point * frames + frame.
 * - `batch_ids` is `[n_rows]`: one id per POINT, in any order (they need not be sorted).  The rows of a point belong to the
 *   point's element, whatever the frame count.
 * - `gamma`, `beta`, `dgamma`, `dbeta` are `[channels]`; `save_mean`, `save_invstd` are `[n_batches, groups]`.
 * - `groups` divides `channels`.  The group of channel `c` is `c % groups`: the reference reshapes its rows to
 *   `(-1, groups)`, so the `channels / groups` channels of a group are STRIDED (`j, j + groups, j + 2 * groups, ...`), not
 *   adjacent.
 * - `n_valid` is NULL (every point is present) or an int32 device word, clamped to `[0, n_rows]`: the present points are
 *   the first `P` of them.  No absent row of `x` or `dy` and no absent id is read; absent rows of `y` and `dx` are `0.0f`.
 * - A present point whose id lies outside `[0, n_batches)` belongs to no element: it enters no sum, and its rows of `y` and
 *   `dx` are `0.0f`.
 * - Every byte of every output is written; nothing depends on what the outputs, the workspace or the absent rows held
 *   before the call.  `n_rows == 0` and `P == 0` are valid.
 *
 * The arithmetic, normatively (tests/group_norm_reference.py restates it in numpy; the kernels meet it bit for bit).
 * "fp32" and "fp64" operations are IEEE operations rounded to nearest even ONE BY ONE: no product is contracted into an
 * addition.  `(double)` of a float and the fp64 product of two floats are exact.
 *
 * Sums.  Chunk `s` covers the points `[s * SE3_GROUP_NORM_CHUNK, (s + 1) * SE3_GROUP_NORM_CHUNK)`: a function of the row
 * index alone, never of `n_rows` or of the word.  A "sum of `u`, `v`" below is this, for every element `b` and channel `c`:
 * - the partials `P1, P2` of `(s, b, c)` start at `+0.0` and add, as fp64 and in ascending row order, `(double)u` and
 *   `(double)v * (double)w` (`v`, `w` floats, stated below) over the present rows of element `b` in chunk `s`;
 * - the channel totals `T1[b, c], T2[b, c]` start at `+0.0` and add the partials in ascending `s`.  A partial is never
 *   `-0.0`, so a chunk without a row of the element is an exact identity -- hence padded equals trimmed;
 * - `counts[b]` is the number of present points of element `b`, and `n = (double)(counts[b] * frames * (channels / groups))`.
 *
 * se3_group_norm_fwd
 * - The sum of `u = x`, `v = w = x` (so `T1 = sum x`, `T2 = sum x * x`).
 * - The group totals `S1[b, j], S2[b, j]` start at `+0.0` and add `T1[b, c]`, `T2[b, c]` over the channels of group `j` in
 *   ascending `c`.
 * - In fp64: `mean = S1 / n`, `var = max(S2 / n - mean * mean, 0)`, `invstd = 1 / sqrt(var + (double)eps)`.  Then
 *   `save_mean[b, j] = (float)mean`, `save_invstd[b, j] = (float)invstd`.  An element without a point gets `0.0f`, `0.0f`.
 *   (The variance is the biased one.  The one-pass form cancels in fp64, where a group with |mean| = 1000 standard deviations
 *   still keeps ten digits of its variance; what such a group loses is the fp32 rounding of `save_mean` itself.)
 * - Row-wise, in fp32, with `m = save_mean[b, c % groups]` and `r = save_invstd[b, c % groups]` of the row's element:
 *   `xhat = (x - m) * r` (a subtraction, then a product), `y = xhat * gamma[c] + beta[c]` (a product, then an addition).
 *
 * se3_group_norm_bwd (`save_mean`, `save_invstd` as the forward call wrote them)
 * - `xhat` is recomputed from `x`, `save_mean`, `save_invstd` exactly as above.
 * - The sum of `u = dy`, `v = dy`, `w = xhat` (so `T1 = sum dy`, `T2 = sum dy * xhat`).
 * - `dbeta[c]` / `dgamma[c]` start at `+0.0` (fp64) and add `T1[b, c]` / `T2[b, c]` in ascending `b`; stored as float.
 * - `A[b, j]` / `Bq[b, j]` start at `+0.0` and add, in fp64, the products `(double)gamma[c] * T1[b, c]` /
 *   `(double)gamma[c] * T2[b, c]` over the channels of group `j` in ascending `c`.  Then `a = (float)(A / n)` and
 *   `q = (float)(Bq / n)` (fp64 divisions, one rounding to float each); an element without a point gets `0.0f`, `0.0f`.
 * - Row-wise, in fp32: `dx = r * ((gamma[c] * dy - a) - xhat * q)`: the product `gamma * dy`, minus `a`, the product
 *   `xhat * q`, the second subtraction, the product with `r` -- five operations, each rounded.
 *
 * Workspace: `se3_group_norm_workspace_bytes(n_rows, frames, n_batches, channels, groups)` bytes serve either call -- 16
 * bytes per (chunk, element, channel) and 4 per (chunk, element), 16 per (element, channel), and a few words per (element,
 * group); 0 for arguments the calls refuse.
 *
 * Errors, all checked on the host before the first launch
 * - a negative `n_rows`, `frames < 1`, `n_batches < 1`, `channels < 1`, `groups < 1`, `channels % groups != 0`, a NULL
 *   required pointer (`gamma`, `beta` of the forward call, `save_mean`, `save_invstd`, `dgamma`, `dbeta`, the workspace;
 *   `x`, `dy`, `batch_ids`, `y` and `dx` when there are rows): SE3_ERR_INVALID_ARGUMENT;
 * - `n_rows * frames * channels >= 2^31` or `n_batches * channels >= 2^31`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_GROUP_NORM_H_
#define SE3CONV_GROUP_NORM_H_

#include <stddef.h>
#include <stdint.h>

/* points per chunk of the order of additions above: a power of two.  Part of the arithmetic contract -- a library built
 * with another value gives other last bits (tests/group_norm_reference.py holds the same number).  It trades the serial
 * chain of one (chunk, element, channel), and the number of such chains the chip can run side by side, against the size of
 * the partial table; 64 is the measured choice among 32 .. 512 for batches with sorted ids (profiles/group_norm.txt). */
#define SE3_GROUP_NORM_CHUNK 64

#ifdef __cplusplus
extern "C" {
#endif

/* host only */
size_t se3_group_norm_workspace_bytes(int64_t n_rows, int32_t frames, int32_t n_batches, int32_t channels, int32_t groups);

int se3_group_norm_fwd(const float* x, const float* gamma, const float* beta, const int32_t* batch_ids, int64_t n_rows,
                       int32_t frames, const int32_t* n_valid, int32_t n_batches, int32_t channels, int32_t groups, float eps,
                       float* y, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, void* stream);

int se3_group_norm_bwd(const float* dy, const float* x, const float* gamma, const float* save_mean, const float* save_invstd,
                       const int32_t* batch_ids, int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t n_batches,
                       int32_t channels, int32_t groups, float* dx, float* dgamma, float* dbeta, void* workspace,
                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_GROUP_NORM_H_ */
