/*
 * se3conv_att_fused.h -- `FeatBasisProj -> se3_basis_att_fwd` and their gradients as one edge-wise operator: the attention of
 * the reference's `MultiHeadAttLayer` / `LoRAttConvLayer` without the aggregate `T [N, 2V, K]`.  `T` is linear in the per-edge
 * embedding `phi`, so scores, attention and output collapse onto per-edge scalars (`c`, `a`, `da`, `dc` below): `T` and `dT`
 * exist nowhere, neither in memory nor in registers.
 *
 * Same conventions as se3conv_basis_att.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, NO atomic on a
 * floating-point number, int status; every error is checked on the host before the first launch).  These entry points are
 * additions inside SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Shapes
 * - `V = value_size >= 1`, `H = num_heads >= 1` with `H | V`, `D = V / H`, `1 <= K = num_basis <= SE3_BASIS_ATT_MAX_BASIS`
 *   (se3conv_basis_att.h: 64).  Head `h` owns the channels `i` in `[h D, (h + 1) D)`; `h(i) = i / D`.
 * - One cloud of `N = n_rows` points: samples and sources are both rows of `x`.  `x [N, 3V]` fp32, dense (row stride `3V`), the
 *   output of the layers' `linear_kqv_`: columns `[0, V)` are the value part `xv`, `[V, 2V)` the query part `xq`, `[2V, 3V)` the
 *   `key`.  `dx [N, 3V]` has the same layout: `dxv | dxq | dkey`.
 * - `neighbors [E, 2]` int32, row `e` = (sample `s_e`, source `p_e`), grouped by sample in ascending sample order;
 *   `ends [N]` int32, inclusive end offsets: the edges of sample `s` are the rows `[ends[s - 1], ends[s])` (`0` for `s = 0`).
 *   Every id lies in `[0, N)`; `ends[N - 1] == E`.  The call does not check what the arrays hold.
 * - `t_samples [E]`, `t_ends [N]`, `t_edge_ids [E]`: the source-major transposition as `se3_csr_transpose` (se3conv.h) writes it
 *   for `n_src = N`, with its third result: entry `j` of source `p`'s group `[t_ends[p - 1], t_ends[p])` is the edge
 *   `t_edge_ids[j]` of `neighbors`, whose sample is `t_samples[j]`.  (se3_csr_transpose orders a group by sample; where a
 *   sample lists one source twice it leaves the order of the twins to the run.  The sums below follow the list they are
 *   handed: the same list, the same bits.)
 * - `phi [E, K]`, `pe [K, V]`, `grad_out [N, V]`, `att [N, K, H]` (the layout `se3_basis_att_fwd` writes), `out [N, V]`,
 *   `dphi [E, K]`, `dpe [K, V]`: fp32, dense.
 * - Arrays need the alignment of their elements (4 bytes) and no more; the workspace is aligned to 16 bytes.  The 16-byte
 *   accesses are taken where `D % 4 == 0` and `x` (for the backward call: and `grad_out`) lies on a 16-byte boundary.
 * - Every byte of every output is written; nothing depends on what the outputs or the workspace held before.  `E == 0` and
 *   `N == 0` are valid (`N == 0` requires `E == 0`): a sample without edges has `s = pe . key` and `out = +0.0`, a source without
 *   incoming edges has `dxv = dxq = +0.0`, and with `N == 0` the backward call writes `dpe = +0.0`.
 *
 * The arithmetic, normatively (tests/att_fused_reference.py restates it in float64 numpy and emulates its order in float32).
 * "fp32" operations are IEEE operations rounded to nearest even; `fma(a, b, c)` is the fused operation, one rounding; exp is
 * the device's fp32 `expf`; `tree_k` is the pairwise sum over `k` of se3conv_basis_att.h.  "Over the edges of `s`" means an fma
 * chain that starts at `+0.0f` and runs in ASCENDING EDGE ORDER; "over the `i` of `h`" one in ascending channel order.  With
 * 16-byte accesses or without, the same operations run in the same order: the two kernel forms give the same bits.
 *
 * se3_att_fused_fwd, per sample `s` and head `h`
 * - `c[e]   = fma(xq[p_e,i], key[s,i], c[e])` over the `i` of `h`, for every edge `e` of `s`.
 * - `s[k]   = fma(phi[e,k], c[e], s[k])` over the edges of `s`; `t[k] = fma(pe[k,i], key[s,i], t[k])` over the `i` of `h`;
 *   `s[k] = s[k] + t[k]`.
 * - `m = max_k s[k]`, `w[k] = exp(s[k] - m)`, `att[k,h] = w[k] / tree_k(w)`.  There is no `1 / sqrt(D)` factor, as in the reference.
 * - `a[e]   = tree_k(phi[e,k] * att[k,h])`, the products rounded to fp32.
 * - `out[s,i] = fma(a[e], xv[p_e,i], out[s,i])` over the edges of `s`, for the `i` of `h`.
 *
 * se3_att_fused_bwd, with `g = grad_out` and `att` as the forward call wrote it.  Per sample `s` and head `h`:
 * - `c[e]` as above; `da[e] = fma(g[s,i], xv[p_e,i], da[e])` over the `i` of `h`.
 * - `datt[k] = fma(phi[e,k], da[e], datt[k])` over the edges of `s`.
 * - `q = tree_k(att[k,h] * datt[k])`, `ds[k] = att[k,h] * (datt[k] - q)` (a subtraction, then a product).
 * - `a[e]` as above; `dc[e] = tree_k(phi[e,k] * ds[k])`.
 * - `dkey[s,i] = r + u` with `r = fma(dc[e], xq[p_e,i], r)` over the edges of `s` and `u = tree_k(ds[k] * pe[k,i])`.
 * Per edge `e` and `k`, over the heads in ascending order from `+0.0f`:
 * - `dphi[e,k] = fma(att[k,h], da[e,h], dphi[e,k])`, then `dphi[e,k] = fma(ds[k,h], c[e,h], dphi[e,k])`.
 * Per source `p` and channel `i`, fma chains from `+0.0f` over the entries `j` of `p`'s group IN THE ORDER OF THE TRANSPOSED
 * LIST, with `e = t_edge_ids[j]` and `s = t_samples[j]`:
 * - `dxv[p,i] = fma(a[e,h(i)], g[s,i], dxv[p,i])`, `dxq[p,i] = fma(dc[e,h(i)], key[s,i], dxq[p,i])`.
 * `dpe[k,i]` is the sum over the points of the fp32 product `ds_n[k,h(i)] * key_n[i]`: chunk `c` covers the points
 * `[c * SE3_ATT_FUSED_CHUNK, (c + 1) * SE3_ATT_FUSED_CHUNK)`; the partial of `(c, k, i)` starts at `+0.0` and adds, as fp64 and
 * in ascending point order, `(double)` of that product; the total starts at `+0.0` and adds the partials in ascending `c`;
 * stored as float -- as se3_basis_att_bwd builds its `dpe`.  Two calls give the same bits.
 *
 * Launches: the forward call is ONE kernel.  The backward call is FOUR: the sample-major pass (recomputes `c`; `da`, `datt`,
 * `ds`, `a`, `dc`, `dphi`, `dkey`; parks `a`, `dc` and `ds` in the workspace), the source-major pass (`dxv`, `dxq`), the chunk
 * partials of `dpe` and their sum (with `N == 0`: the sum alone).  Five launches for a forward and a backward call.
 *
 * Workspace: `se3_att_fused_workspace_bytes(n_rows, n_edges, value_size, num_heads, num_basis)` bytes serve se3_att_fused_bwd:
 * `a [E,H]` and `dc [E,H]` (fp32, each rounded up to a multiple of 16 bytes), `ds [N,K,H]` (fp32, rounded up likewise), then 8
 * bytes per (chunk, k, i), one chunk when `n_rows == 0`; 0 for arguments the calls refuse.  The forward call needs none.
 *
 * Errors, all checked on the host before the first launch
 * - a negative count, `n_edges > 0` with `n_rows == 0`, `value_size < 1`, `num_heads < 1`, `num_heads` not dividing `value_size`,
 *   `num_basis < 1`, a NULL required pointer (`pe`; `dpe` and the workspace; `x`, `ends`, `att`, `out`, `grad_out`, `dx`, `t_ends`
 *   when `n_rows > 0`; `phi`, `neighbors`, `dphi`, `t_samples`, `t_edge_ids` when `n_edges > 0`): SE3_ERR_INVALID_ARGUMENT (-1);
 * - `num_basis > SE3_BASIS_ATT_MAX_BASIS`, or one of `N * 3V`, `N * K * H`, `E * K`, `E * H`, `E * 2`, `K * V` at or beyond `2^31`:
 *   SE3_ERR_UNSUPPORTED (-2);
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE (-3).
 */
#ifndef SE3CONV_ATT_FUSED_H_
#define SE3CONV_ATT_FUSED_H_

#include <stddef.h>
#include <stdint.h>

/* points per chunk of the order of additions of `dpe`: a multiple of 64.  Part of the arithmetic contract
 * (tests/att_fused_reference.py holds the same number). */
#define SE3_ATT_FUSED_CHUNK 256
/* edges of a sample a wavefront holds at a time: a sample of any degree is walked in slabs of this many edges.  Not part of
 * the arithmetic (the chains run in ascending edge order across slabs). */
#define SE3_ATT_FUSED_SLAB 64

#ifdef __cplusplus
extern "C" {
#endif

/* host only */
size_t se3_att_fused_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t value_size, int32_t num_heads, int32_t num_basis);

int se3_att_fused_fwd(const float* phi, const float* x, const float* pe, const int32_t* neighbors, const int32_t* ends,
                      int64_t n_rows, int64_t n_edges, int32_t value_size, int32_t num_heads, int32_t num_basis, float* att,
                      float* out, void* stream);

int se3_att_fused_bwd(const float* grad_out, const float* phi, const float* x, const float* pe, const float* att,
                      const int32_t* neighbors, const int32_t* ends, const int32_t* t_samples, const int32_t* t_ends,
                      const int32_t* t_edge_ids, int64_t n_rows, int64_t n_edges, int32_t value_size, int32_t num_heads,
                      int32_t num_basis, float* dphi, float* dx, float* dpe, void* workspace, size_t workspace_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_ATT_FUSED_H_ */
