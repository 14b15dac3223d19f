/*
 * se3conv_augment.h -- the augmentation pipeline of libse3conv_hip.so: what point_cloud_lib/augment/ of the reference does
 * to ONE scene on the host, done to a whole batch on the device.  Every batch element is augmented on its own, every random
 * choice comes from numbers the caller supplies (`draws`) or from a counter-based hash of a seed word, crops write into
 * padded clouds and leave the surviving count in a device word.  ElasticDistortionAug has no entry point here: se3conv_elastic.h.
 *
 * Same conventions as se3conv.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, capturable into a HIP graph, no memset calls, int status).  These
 * entry points are additions inside SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Contract
 *
 * - Rows and elements.
 *   - The present rows are the first `min(n_rows, *n_valid)` (`n_valid` NULL: all `n_rows`; the word is clamped to
 *     `[0, n_rows]`).  Nothing is read from a row behind the count.  Every byte of every output is written; output rows behind
 *     the count are zero.
 *   - `batch_ids` is non-decreasing on the present rows.  Element `b` is the run of present rows with `batch_ids == b`, found
 *     by binary search; `start_b` is its first row, `n_b` its length.  Rows with an id outside `[0, n_batches)` belong to no
 *     element: the row-wise calls treat them like rows of an element whose table is the identity, whose gate is closed.
 * - fp32 arithmetic is "plain": every operation rounded on its own, no fused multiply-add.  fp64 likewise.
 * - Affine table.  `affine [n_batches,12]` fp32 holds `M` (row-major 3 x 3) and `t` (3) per element: `y = x M + t`,
 *   `y_j = (((x_0 M_0j) + (x_1 M_1j)) + (x_2 M_2j)) + t_j`.  A NULL table is the identity (`y = x`, no arithmetic).
 * - Draws.  `draws [n_batches, SE3_AUG_DRAWS]` fp32 uniform numbers in [0,1); `u_k` is column `k` of the element's row.
 *   `u_0` is the gate of a step: the step applies to the element iff `u_0 <= p_prob` (the reference's
 *   `torch.rand(1).item() <= prob_` per scene); otherwise the element keeps its table / all its rows / gets no noise.
 * - Hash.  `mix` and `h(seed, s, p) = mix((mix(seed ^ mix(s)) + p*0x9E3779B9) mod 2^32)` are those of se3conv_capped.h.
 *   `seed_eff = (seed + (seed_device ? *seed_device : 0)) mod 2^32`.  The word of (step, row, j) is
 *   `w(step, row, j) = mix((h(seed_eff, step, row) + (j+1)*0x9E3779B9) mod 2^32)`; its uniform number is
 *   `U(w) = (w >> 8) * 2^-24` in [0,1).  `row` is the row's index in the arrays of the call.  Check vectors
 *   `(seed_eff, step, row, j) -> w`:
 *     (0,0,0,0) -> 0x92ca2f0e      (1,2,3,0) -> 0x93192184      (12345,7,99999,5) -> 0x86f1df33
 *
 * se3_aug_stats
 * - Of `y = x M_b + t_b` (never stored) per element: `counts[b] = n_b`, `stats[b] = [min 3 | max 3 | mean 3 | std 3]`.
 * - The element's rows are cut into chunks of SE3_AUG_CHUNK rows from `start_b`.  Per chunk and coordinate, `(double)y` and
 *   `(double)y * (double)y` are laid into SE3_AUG_CHUNK slots (0.0 for the slots behind the chunk's rows) and folded by the
 *   tree `for s = CHUNK/2, CHUNK/4, .., 1: slot[i] += slot[i + s] (i < s)`; the chunk sums are added in ascending chunk order
 *   starting from 0.0.  `mean = (float)(S1 / n)`, `std = (float)sqrt(max((S2 - S1*S1/n) / (n - 1), 0))` in fp64 (unbiased,
 *   `torch.std`; NaN for `n_b = 1`, as there).  No atomic on a floating-point number: two calls give the same bits, a
 *   padded call those of the trimmed call.
 * - `n_b = 0`: count 0 and twelve zeros.
 * - min and max are `fminf` / `fmaxf` folds: a NaN coordinate of a present row is left out of the bounds (torch's amin / amax
 *   would hand it on) and makes the mean and std of its column NaN.
 *
 * se3_aug_affine_step
 * - One thread per element builds the step's `(A, s)` (3 x 3, 3) and replaces the table by `M' = M A`, `t' = t A + s`:
 *   `M'_ij = ((M_i0 A_0j) + (M_i1 A_1j)) + (M_i2 A_2j)`, `t'_j = (((t_0 A_0j) + (t_1 A_1j)) + (t_2 A_2j)) + s_j`.  Gate
 *   closed: the twelve words stay as they are, bit for bit.
 * - `consts` (host, SE3_AUG_CONSTS doubles) per kind; "fp32(c)" is the constant rounded to fp32 on the host side of the call:
 *   - SE3_AUG_ROT_AXIS: [axis, min, max, fixed].  `angle = fixed ? min : (double)u_1 * (max - min) + min` in fp64;
 *     `c = cos(angle)`, `s = sin(angle)` in fp64, rounded once.  axis 0: A = [[1,0,0],[0,c,-s],[0,s,c]]; axis 1:
 *     [[c,0,s],[0,1,0],[-s,0,c]]; axis 2: [[c,-s,0],[s,c,0],[0,0,1]] (RotationAug.py:55-77).
 *   - SE3_AUG_ROT_3D: [axis].  axis >= 0: as above with `angle = ((double)u_1 * 2) * pi`.  axis < 0: four normal numbers
 *     `g_0 = r_a cos(2 pi u_2)`, `g_1 = r_a sin(2 pi u_2)`, `r_a = sqrt(-2 log(1 - u_1))`, `g_2, g_3` likewise from
 *     `u_3, u_4`, all fp64; `q = g / copysign(|g|, g_0)`; A is the matrix of quaternion `q` (real part first), fp64, rounded once.
 *   - SE3_AUG_CENTER: [ax_0, ax_1, ax_2].  A = I, `s_j = ax_j ? -mean_j : 0`.
 *   - SE3_AUG_LINEAR: [range_a, min_a, range_b, min_b, single, fixed, a_0..2, b_0..2] (SE3_AUG_CONSTS = 12).
 *     `a_j = (u_{1+k} fp32(range_a)) + fp32(min_a)`, `b_j = (u_{4+k} fp32(range_b)) + fp32(min_b)`, `k = single ? 0 : j`;
 *     fixed: `a_j, b_j = fp32(consts[6+j]), fp32(consts[9+j])`.  A = diag(a), s = b.
 *   - SE3_AUG_MIRROR: [mirror_prob, ax_0, ax_1, ax_2].  A = diag(m), `m_j = (ax_j && u_{1+j} > fp32(mirror_prob)) ? -1 : 1`.
 *   - SE3_AUG_TRANSLATION: [ratio_0, ratio_1, ratio_2].  A = I, `s_j = ((max_j - min_j) / 2) * (((u_{1+j} * 2) - 1) * fp32(ratio_j))`.
 *   - SE3_AUG_STDNORM: [new_std].  A = diag(k, k, k), `k = fp32(new_std) / max_j std_j`.
 *   `counts` / `stats` are those of se3_aug_stats of the cloud under the table as it is before the step (kinds CENTER,
 *   TRANSLATION, STDNORM; NULL for the others).
 *
 * se3_aug_apply
 * - `y = x M_b + t_b` per present row (`linear_only`: without `t_b`), in the order above; `y` may be `x`.
 * - Noise (`noise_draws` not NULL; NoiseAug.py:50-54): for an element with `noise_draws[b][0] <= noise_prob`, channel `c`:
 *   `z = sqrtf(-2 logf(1 - U(w(step,row,2c)))) * cosf(2 pi U(w(step,row,2c+1)))` in fp32, `e = z * noise_sigma`, clipped to
 *   `[-noise_clip, noise_clip]` when `noise_clip >= 0`, and `y_c += e * noise_scale` last.  `noise_scale` is 1 for the points;
 *   a flagged extra tensor gets the points' clipped noise times sigma once more (`cur_tensor + cur_noise*self.stddev_`,
 *   NoiseAug.py:58-61): the same seed, step and rows with `noise_scale = noise_sigma`.
 * - `ones_mask [n_rows]` bytes (may be NULL): a present row whose byte is 0 is written as (1, 1, 1) (DropAug.py:53-54).
 *
 * se3_aug_keep_mask writes one byte per row, 1 = keep; 0 for absent rows; gate closed: the element keeps every row.
 *   - SE3_AUG_DROP: [drop_prob, j].  Keep iff `U(w(step,row,j)) > fp32(drop_prob)` (DropAug.py:51), `0 <= j <= 5`.  DropAug
 *     uses `j = 0`; the other words are those se3_aug_apply's noise reads, which a test pins bit for bit through this mask.
 *   - SE3_AUG_CROP_BOX: [range, min_size].  `size_j = min((u_{1+j} fp32(range)) + fp32(min_size), max_j - min_j)`,
 *     `lo_j = (u_{4+j} ((max_j - size_j) - min_j)) + min_j`; keep iff `x_j >= lo_j && x_j <= lo_j + size_j` for all `j`
 *     (CropBoxAug.py:50-69).  ONE draw: the reference draws again while no point survives, here such an element is empty.
 *   - SE3_AUG_CROP_PTS: [max_pts, crop_ratio].  `m_b = min(max_pts > 0 ? max_pts : n_b, (int)((double)n_b * crop_ratio))`;
 *     `n_b <= m_b`: everything kept.  Else the anchor is row `start_b + min((int)floorf(u_1 * n_b), n_b - 1)` and the `m_b` rows
 *     with the smallest `d = ((dx dx) + (dy dy)) + (dz dz)` (fp32) are kept, ties to the lowest row (CropPtsAug.py:50-59,
 *     whose argsort leaves ties open).  The selection is a radix select on the bits of `d` (4 passes of 8 bits, one
 *     workgroup per element), not a sort.
 *   `stats` of se3_aug_stats with a NULL table (CROP_BOX; else NULL).
 *
 * se3_aug_compact
 * - `idx [n_rows]`: the rows with `mask != 0` among the present rows in ascending order, -1 behind them.  `n_out[0]` their
 *   number, `counts_out[b]` the number per element.  The rows themselves follow through se3_rows_gather_padded.
 * - `idx_orig [n_rows]` (optional): `idx_in[idx[i]]` where `idx[i] >= 0`, else -1: the composition with an earlier
 *   compaction whose `idx` is `idx_in` (`idx_in` NULL: a copy of `idx`).
 *
 * Errors, decided on the host before the first launch: `n_rows < 0`, `n_batches < 1`, an unknown kind, an axis outside
 * 0..2, a word index outside 0..5, missing `consts` / `draws` / `counts` / `stats` for a kind that needs them, a NULL
 * `counts` / `stats` / `n_out` / `counts_out` / `affine` (in-out) / workspace, and with `n_rows > 0` a NULL `pts` / `x` /
 * `batch_ids` / `y` / `mask` / `idx`: SE3_ERR_INVALID_ARGUMENT; `n_rows >= 2^31`: SE3_ERR_UNSUPPORTED; `workspace_bytes`
 * below the query's value: SE3_ERR_WORKSPACE.  The per-row arrays are not looked at when `n_rows == 0`: se3_aug_apply and
 * se3_aug_keep_mask then return SE3_OK without a launch, whatever their pointers.  The optional inputs of se3_aug_apply
 * (`affine`, `noise_draws`, `seed_device`, `ones_mask`) are absent when NULL and otherwise taken as given.
 * Grids are sized from `n_rows` and `n_batches`; none is capped.  The first launch of se3_aug_stats lays out the chunk
 * slots with ONE thread's loop over `n_batches` (a few microseconds per thousand elements): meant for batches of up to some
 * thousand elements, correct for any.
 */
#ifndef SE3CONV_AUGMENT_H_
#define SE3CONV_AUGMENT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3_AUG_CHUNK 256  /* rows per chunk of the order of additions of se3_aug_stats */
#define SE3_AUG_DRAWS 8    /* uniform numbers per (step, element) */
#define SE3_AUG_CONSTS 12  /* doubles per step */

enum se3_aug_kind {
  SE3_AUG_ROT_AXIS = 0, SE3_AUG_ROT_3D = 1, SE3_AUG_CENTER = 2, SE3_AUG_LINEAR = 3, SE3_AUG_MIRROR = 4,
  SE3_AUG_TRANSLATION = 5, SE3_AUG_STDNORM = 6,                      /* se3_aug_affine_step */
  SE3_AUG_DROP = 16, SE3_AUG_CROP_BOX = 17, SE3_AUG_CROP_PTS = 18   /* se3_aug_keep_mask */
};

/* element and chunk boundaries and six fp64 sums + six fp32 bounds per chunk; 0 for invalid arguments */
size_t se3_aug_stats_workspace_bytes(int64_t n_rows, int32_t n_batches);

int se3_aug_stats(const float* pts,            /* [n_rows,3] */
                  const int32_t* batch_ids,    /* [n_rows] */
                  int64_t n_rows,
                  const int32_t* n_valid,      /* device word, may be NULL */
                  int32_t n_batches,           /* host */
                  const float* affine,         /* [n_batches,12], may be NULL = identity */
                  int32_t* counts,             /* [n_batches] */
                  float* stats,                /* [n_batches,12] */
                  void* workspace, size_t workspace_bytes, void* stream);

int se3_aug_affine_step(int32_t kind,           /* host */
                        const double* consts,   /* host [SE3_AUG_CONSTS] */
                        float prob,             /* host */
                        const float* draws,     /* [n_batches, SE3_AUG_DRAWS] */
                        const int32_t* counts,  /* [n_batches], kinds that need statistics */
                        const float* stats,     /* [n_batches,12], kinds that need statistics */
                        int32_t n_batches,
                        float* affine,          /* [n_batches,12], in and out */
                        void* stream);

int se3_aug_apply(const float* x, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid, int32_t n_batches,
                  const float* affine,          /* may be NULL = identity */
                  int32_t linear_only,          /* host */
                  const float* noise_draws,     /* [n_batches, SE3_AUG_DRAWS], may be NULL = no noise */
                  float noise_prob, float noise_sigma, float noise_clip,   /* host; noise_clip < 0: no clip */
                  float noise_scale,            /* host; 1 for the points, sigma for an extra tensor */
                  uint32_t seed, const uint32_t* seed_device, uint32_t step,
                  const uint8_t* ones_mask,     /* [n_rows], may be NULL */
                  float* y,                     /* [n_rows,3] */
                  void* stream);

int se3_aug_keep_mask(int32_t kind, const double* consts, float prob, const float* pts, const int32_t* batch_ids,
                      int64_t n_rows, const int32_t* n_valid, int32_t n_batches, const float* draws,
                      const float* stats,       /* [n_batches,12], SE3_AUG_CROP_BOX */
                      uint32_t seed, const uint32_t* seed_device, uint32_t step,
                      uint8_t* mask,            /* [n_rows] */
                      void* stream);

/* the scanned mask and the scan's own temporary; 0 for invalid arguments */
size_t se3_aug_compact_workspace_bytes(int64_t n_rows);

int se3_aug_compact(const uint8_t* mask, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid,
                    int32_t n_batches,
                    const int32_t* idx_in,      /* [n_rows], may be NULL */
                    int32_t* idx,               /* [n_rows] */
                    int32_t* idx_orig,          /* [n_rows], may be NULL */
                    int32_t* n_out,             /* [1] */
                    int32_t* counts_out,        /* [n_batches] */
                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_AUGMENT_H_ */
