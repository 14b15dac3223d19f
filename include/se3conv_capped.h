/*
 * se3conv_capped.h -- the capped ball query of libse3conv_hip.so: max_neighbors > 0 of
 * point_cloud_lib_ops.ball_query (custom_ops/ball_query/store_neighbors.cu:46-114) as a seeded, order-free random
 * subset.  The reference draws its subset with atomics and a seed from time(NULL): it is neither uniform nor
 * repeatable.  The rule below is deterministic and uniform.
 *
 * Same conventions as se3conv.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, capturable into a HIP graph, no memset calls, int status).  These
 * entry points are additions inside SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Contract
 *
 * `N(s)` is the source set the uncapped query finds for sample `s`. The predicate and the batch test are the same, bit for bit. `c = |N(s)|`.
 *
 * - `m <= 0` or `c <= m`: keep `N(s)`. This matches the reference ("zero or less" means no limit).
 * - Otherwise: keep the `m` sources `p ∈ N(s)` with the smallest 64-bit keys `key(s,p) = (uint64(h) << 32) | uint32(p)`.
 * - `mix(x)` is the murmur3 finaliser on 32 bits: `x^=x>>16; x*=0x85ebca6b; x^=x>>13; x*=0xc2b2ae35; x^=x>>16`.
 * - `h = mix((mix(seed_eff ^ mix(s)) + p*0x9E3779B9) mod 2^32)`.
 * - `seed_eff = (seed + (seed_device ? *seed_device : 0)) mod 2^32`.
 * - `s` and `p` are indices into the caller's arrays, not sorted positions.
 * - Check vectors `(seed, s, p) -> h`:
 *   - `(0,0,0) -> 0x0`
 *   - `(1,2,3) -> 0x69157d8e`
 *   - `(12345,65535,99999) -> 0x044b2766`
 *   - `(0xFFFFFFFF,1499,5999) -> 0x72c91147`
 *
 * The kept set depends only on `(seed_eff, s, N(s))`. It is therefore the same through every search path: 64-bit-key grid, 32-bit-key grid, all-pairs with and without the inline prefix, and a shared source grid with `grid_valid` 0 or 1.
 *
 * Output:
 *
 * - Rows are grouped by sample in ascending sample order.
 * - Inside a sample the survivors keep the order the uncapped query lists them in. With `m >= max c` the result is therefore bit-identical to `se3_ball_query_bounded`.
 * - `ends` holds the inclusive offsets of `min(c, m)`.
 * - `degrees [n_dst]` is optional and may be NULL. When given it receives `c`.
 * - `info[0]` is the number of kept edges. `info[1]` is the overflow flag against `capacity`. The truncation rules are those of `se3_ball_query_bounded`.
 *
 * Limit: 1 <= max_neighbors <= 64 (one kept key per lane of the wavefront that owns the sample).  max_neighbors > 64
 * returns SE3_ERR_UNSUPPORTED; there is no general selection.
 *
 * With capacity = n_dst * max_neighbors the edge buffer can never overflow.
 *
 * A source-major list of a capped neighbourhood is the transposition of this very list (se3_csr_transpose_bounded with
 * n_valid = info): a second query with the clouds' roles swapped draws another subset, and the capped graph of a cloud
 * against itself is NOT symmetric, so `sources` is not the list se3conv_bwd wants.
 */
#ifndef SE3CONV_CAPPED_H_
#define SE3CONV_CAPPED_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* se3_ball_query_workspace_bytes(n_src, n_dst) plus one 64-bit threshold per sample */
size_t se3_ball_query_capped_workspace_bytes(int64_t n_src, int64_t n_dst);

/* The arguments of se3_ball_query_bounded_shared (se3conv.h), with the same meaning, then the cap.
 *   grid (may be NULL = no shared grid: the source cloud's grid is built inside the workspace; grid_bytes and grid_valid
 *     are then ignored);
 *   max_neighbors (host): m of the contract;
 *   seed (host), seed_device (1 word, may be NULL): a captured graph draws fresh subsets on every replay when the caller
 *     updates *seed_device between replays;
 *   degrees [n_dst] int32 (optional): the uncapped degree c of every sample.
 * Passes: count, threshold (samples with c > m only recompute their hits and keep the m smallest keys: a bitonic sort
 * of each 64-candidate chunk, a min-merge against the kept list and six merge stages, skipped for chunks without a key
 * below the current threshold), scan, store. */
int se3_ball_query_capped(const float* pts_src, const float* pts_dst, const int32_t* batch_src,
                          const int32_t* batch_dst, const float* aabb_min, const int32_t* num_cells, float radius,
                          int64_t n_src, int64_t n_dst, int32_t n_batches, void* grid, size_t grid_bytes,
                          int32_t grid_valid, void* workspace, size_t workspace_bytes, int64_t capacity,
                          int32_t* neighbors, int32_t* sources, int32_t* ends, int32_t* info, void* stream,
                          int32_t max_neighbors, uint32_t seed, const uint32_t* seed_device, int32_t* degrees);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_CAPPED_H_ */
