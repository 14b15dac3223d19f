/*
 * se3conv_elastic.h -- ElasticDistortionAug of the reference (point_cloud_lib/augment/ElasticDistortionAug.py) on a batch, on the
 * device: per (element, octave) a 3-channel grid of Gaussian numbers sized by the element's box, blurred by six 3-tap box
 * passes, and per point a trilinear look-up per octave, each octave at the coordinates the octave before it moved.  The step
 * is not affine: it has kernels of its own and a caller-sized grid buffer, and it does not fold into the tables of
 * se3conv_augment.h, whose conventions (rows and elements, the gate, "plain" fp32, the hash, the draws) hold here word for word.
 *
 * Same conventions as se3conv.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, no allocation, capturable into a HIP graph, no memset calls, int status).
 * These entry points are additions inside SE3_ABI_VERSION 6.  No atomic on a floating-point number anywhere: two calls give
 * the same bits, a padded cloud (`n_valid`) the bits of the trimmed one, and absent rows are never read.
 *
 * Contract
 *
 * se3_elastic_plan
 * - `counts [B]`, `stats [B,12]` (min 3 | max 3 | ..): those of se3_aug_stats of the cloud as it is in front of the step;
 *   `draws [B, SE3_AUG_DRAWS]`; `granularity` host `[n_octaves]`, `g_l = fp32(granularity[l])`.
 * - Element `b` is OPEN iff `u_0 <= prob` and `counts[b] > 0`.
 * - The quotient of (b, l, j) is `q = (max_j - min_j) / g_l` in fp32.  The box of an open element is FINITE iff every one of
 *   its `3 n_octaves` quotients satisfies `0 <= q < SE3_ELASTIC_MAX_QUOTIENT` (false for NaN, for an infinite bound, and for
 *   a column of NaN coordinates, whose bounds se3_aug_stats leaves at +inf / -inf).
 * - `grid_table int64 [B, n_octaves, 4] = (nx, ny, nz, offset)`.  Open and finite: `n_j = (int)floorf(q) + 3`
 *   (ElasticDistortionAug.py:63-67); every other element: three zeros.
 * - `offset`: the exclusive prefix, in int64, of `cells = nx*ny*nz` over the entries of the open, finite elements,
 *   element-major, octave-minor.  An entry is PLACED iff `offset + cells <= grid_capacity`; as the prefix only grows, no
 *   entry behind the first that is not placed is placed either.  An element is DISTORTED iff it is open, finite, and all its
 *   octaves are placed.  Every entry of an element that is not distorted is written with offset -1; the distorted elements
 *   are therefore a run of the open, finite ones from the front, and the PLACED TOTAL is the sum of their cells.
 * - `overflow int32 [1]` is written on every call: bit 0 iff an open, finite element is not distorted (no room), bit 1 iff
 *   an open element's box is not finite.
 * - The workspace (se3_elastic_workspace_bytes) receives `tile_prefix int64 [B * n_octaves + 1]`: the exclusive prefix of
 *   `ceil(nx/T) ceil(ny/T) ceil(nz/T)`, `T = SE3_ELASTIC_TILE`, over the entries of distorted elements (0 for the others), and
 *   the total in the last word.  It is what se3_elastic_grids deals its tiles by; every word of it is written.
 * - One workgroup; its prefix is ONE thread's loop over `B * n_octaves` entries, as the slot layout of se3_aug_stats.
 *
 * se3_elastic_grids
 * - `grid float [grid_capacity, 4]`, 16-byte aligned.  Cell `(ix, iy, iz)` of a placed entry of a distorted element is row
 *   `offset + q`, `q = (ix*ny + iy)*nz + iz`; lanes 0..2 are the channels (the displacement along x, y, z), lane 3 is 0.0f.
 *   Nothing else is written: not the rows behind the placed total, nothing past `grid_capacity`.
 * - Raw numbers.  `seed_eff` as in se3conv_augment.h; `seed_bl = h(seed_eff, step, b * SE3_ELASTIC_MAX_OCTAVES + l)`; the raw
 *   number of cell `q`, channel `c` is `sqrtf(-2 logf(1 - U(w_bl(q, 2c)))) * cosf(2 pi U(w_bl(q, 2c+1)))` with
 *   `w_bl(q, j) = mix((h(seed_bl, 0, q mod 2^32) + (j+1)*0x9E3779B9) mod 2^32)`: the Gaussian number of se3_aug_apply with
 *   seed `seed_bl`, step 0, row `q`.  An element's field depends on (seed, seed word, step, b, l, its own dims) and on
 *   nothing else in the batch.  `noise_in [grid_capacity, 4]` (may be NULL) holds raw numbers in the layout of `grid`
 *   (lane 3 is not read) and replaces the hash.
 * - Blur.  One pass along axis `a`: `out[i] = ((in[i-1]*t + in[i]*t) + in[i+1]*t)`, `t = fp32(1/3)`, `i` the index along
 *   `a`, a neighbour outside the grid 0.0f; every operation one fp32 rounding, no contraction.  Six passes: x, y, z, x, y, z
 *   (`conv3d(.., padding='same', groups=3)` with kernels of 1/3, :57-59, :72-75).
 * - One workgroup per tile of T^3 cells: the tile and a halo of 2 are generated into LDS (out-of-grid cells 0.0f), the six
 *   passes run there on regions that shrink by one per pass and axis, out-of-grid cells forced back to 0.0f after each, and
 *   the tile is stored once, 16 bytes per cell.  A cell's value is the same sequence of operations whatever the tiling.  A
 *   fixed number of workgroups strides over `tile_prefix`'s total and finds each tile's entry by binary search.
 *
 * se3_elastic_displace
 * - One thread per row, `y [n_rows,3]`; absent rows come out zero; a present row whose id is outside `[0, n_batches)` or
 *   whose element is not distorted (offset < 0) is copied bit for bit.
 * - Else `c = x`, and for octave `l = 0 .. n_octaves-1` in turn, with `min`, `max` of `stats` (the box in front of the step,
 *   not of the moved points, :61-63, :78) and `n` of the table:
 *     `p_j = ((c_j - min_j) / (max_j - min_j)) * (float)(n_j - 1)`, `p_j = 0` where `max_j == min_j` (the reference divides
 *       0 by 0 there and returns NaN for the whole cloud; a planar cloud is displaced here), then `p_j = fminf(fmaxf(p_j, 0),
 *       (float)(n_j - 1))` (`padding_mode='border'`, `align_corners=True`; a NaN becomes 0);
 *     `i_j = min((int)floorf(p_j), n_j - 2)`, `f_j = p_j - (float)i_j`;
 *     `s_c = 0`, and over the 8 corners in lexicographic `(dx, dy, dz)` order: `w = (wx*wy)*wz`, `w_j = dj ? f_j : 1 - f_j`,
 *       `s_c = s_c + w * G_c(i_x + dx, i_y + dy, i_z + dz)`;
 *     `c_c = c_c + s_c * fp32(magnitude[l])`.
 *   Grid axis 0 goes with x, 1 with y, 2 with z: what the reference's swap of columns 0 and 2 in front of `grid_sample`
 *   amounts to.  `y = c` after the last octave.
 *
 * Errors, decided on the host before the first launch: `n_octaves` outside `1..SE3_ELASTIC_MAX_OCTAVES`, `n_batches < 1`,
 * `n_rows < 0`, a granularity that is not `> 0`, `grid_capacity < 0`, a NULL `counts` / `stats` / `draws` / `granularity` /
 * `magnitude` / `grid_table` / `overflow` / workspace, a NULL `grid` with `grid_capacity > 0`, and with `n_rows > 0` a NULL
 * `x` / `batch_ids` / `y` / `grid`: SE3_ERR_INVALID_ARGUMENT; `n_rows >= 2^31`: SE3_ERR_UNSUPPORTED; `workspace_bytes` below the
 * query's value: SE3_ERR_WORKSPACE.  `n_rows == 0`: se3_elastic_displace returns SE3_OK without a launch.
 */
#ifndef SE3CONV_ELASTIC_H_
#define SE3CONV_ELASTIC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3_ELASTIC_MAX_OCTAVES 4          /* the reference's lists use 3 */
#define SE3_ELASTIC_TILE 8                 /* edge of the blur kernel's output tile, in cells */
#define SE3_ELASTIC_MAX_QUOTIENT 1048576   /* 2^20: extent / granularity at and above which a box counts as not finite */

/* the tile prefix; 0 for invalid arguments */
size_t se3_elastic_workspace_bytes(int32_t n_batches, int32_t n_octaves);

int se3_elastic_plan(const int32_t* counts,       /* [n_batches] */
                     const float* stats,          /* [n_batches,12] */
                     const float* draws,          /* [n_batches, SE3_AUG_DRAWS] */
                     float prob,                  /* host */
                     const double* granularity,   /* host [n_octaves] */
                     int32_t n_octaves, int32_t n_batches,
                     int64_t grid_capacity,       /* host, cells */
                     int64_t* grid_table,         /* [n_batches, n_octaves, 4] */
                     int32_t* overflow,           /* [1] */
                     void* workspace, size_t workspace_bytes, void* stream);

int se3_elastic_grids(const int64_t* grid_table, int32_t n_batches, int32_t n_octaves, int64_t grid_capacity,
                      uint32_t seed, const uint32_t* seed_device, uint32_t step,
                      const float* noise_in,      /* [grid_capacity,4], may be NULL = the hash */
                      float* grid,                /* [grid_capacity,4] */
                      void* workspace, size_t workspace_bytes,   /* as se3_elastic_plan left it */
                      void* stream);

int se3_elastic_displace(const float* x, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid, int32_t n_batches,
                         const float* stats, const int64_t* grid_table, int32_t n_octaves,
                         const double* magnitude, /* host [n_octaves] */
                         const float* grid,       /* [grid_capacity,4] */
                         float* y,                /* [n_rows,3] */
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_ELASTIC_H_ */
