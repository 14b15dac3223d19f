/*
 * se3conv_basis_att.h -- the attention stage of the reference's `MultiHeadAttLayer` and `LoRAttConvLayer`: per point and per
 * head a softmax over the K basis functions of what `se3_feat_basis_proj` aggregated, read in that operator's own layout
 * (no transposed copy, no `N x K x V` intermediate besides the inputs and outputs named here).
 *
 * Same conventions as se3conv_pne.h (extern "C", device pointers unless marked "host", caller-owned outputs and workspace,
 * asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, no atomics, int
 * status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Shapes
 * - `V = value_size >= 1`, `H = num_heads >= 1` with `H | V`, `D = V / H`, `1 <= K = num_basis <= SE3_BASIS_ATT_MAX_BASIS`.  Head
 *   `h` owns the channels `i` in `[h D, (h + 1) D)`; `h(i) = i / D`.
 * - `T [N, 2V, K]` fp32, as `se3_feat_basis_proj` writes it for `2V` channels: rows `[0, V)` of a point are the value part
 *   `Tv[i,k]`, rows `[V, 2V)` the query part `Tq[i,k]`.  `dT` has the same layout.
 * - `key`: `N` rows of `V` floats, row `n` at `key + n * key_stride` (`key_stride >= V`, in floats; the floats between rows are
 *   never read).  `pe [K,V]`, `grad_out [N,V]`, `att [N,K,H]`, `out [N,V]`, `dkey [N,V]` (dense), `dpe [K,V]`.
 * - Every byte of every output is written; nothing depends on what the outputs or the workspace held before.  `n_rows == 0`
 *   is valid (the forward call writes nothing, the backward call writes `dpe = +0.0`).
 *
 * The arithmetic, normatively (tests/basis_att_reference.py restates it in float64 numpy).  "fp32" operations are IEEE
 * operations rounded to nearest even; `fma(a, b, c)` is the fused operation, one rounding; exp is the device's fp32 `expf`.
 * `tree_k(x)` is the pairwise sum over `k`: with `P` the smallest power of two `>= K` and `x[k] = +0.0f` for `K <= k < P`,
 * level after level `x[j] = x[2j] + x[2j + 1]` (fp32) until one value is left.  It does not depend on which kernel form runs.
 *
 * se3_basis_att_fwd, per point `n` and head `h`
 * - `s[k] = +0.0f`, then `s[k] = fma(Tq[i,k] + pe[k,i], key[i], s[k])` (an addition, then the fma) over the `i` of `h`, ascending.
 * - `m = max_k s[k]`, `e[k] = exp(s[k] - m)`, `att[k,h] = e[k] / tree_k(e)`.  There is no `1 / sqrt(D)` factor, as in the reference.
 * - `out[i] = tree_k(Tv[i,k] * att[k,h(i)])`, the products rounded to fp32.
 *
 * se3_basis_att_bwd, per point `n` and head `h`, with `g = grad_out` and `att` as the forward call wrote it
 * - `datt[k] = +0.0f`, then `datt[k] = fma(g[i], Tv[i,k], datt[k])` over the `i` of `h`, ascending.
 * - `q = tree_k(att[k,h] * datt[k])`, `ds[k] = att[k,h] * (datt[k] - q)` (a subtraction, then a product).
 * - `dTv[i,k] = g[i] * att[k,h(i)]`, `dTq[i,k] = ds[k] * key[i]`, `dkey[i] = tree_k(ds[k] * (Tq[i,k] + pe[k,i]))`.
 * - `dpe[k,i]` is the sum over the points of `dTq[i,k]` as stored (the fp32 product `ds_n[k,h(i)] * key_n[i]`): chunk `c` covers
 *   the points `[c * SE3_BASIS_ATT_CHUNK, (c + 1) * SE3_BASIS_ATT_CHUNK)`; the partial of `(c, k, i)` starts at `+0.0` and adds,
 *   as fp64 and in ascending point order, `(double)dTq_n[i,k]`; the total starts at `+0.0` and adds the partials in ascending
 *   `c`; stored as float.  Two calls give the same bits.
 *
 * Workspace: `se3_basis_att_workspace_bytes(n_rows, value_size, num_heads, num_basis)` bytes serve se3_basis_att_bwd -- 8 bytes
 * per (chunk, k, i), one chunk when `n_rows == 0`, and nothing else; 0 for arguments the calls refuse.  The forward call needs none.
 *
 * Errors, all checked on the host before the first launch
 * - a negative count, `value_size < 1`, `num_heads < 1`, `num_heads` not dividing `value_size`, `num_basis < 1`,
 *   `key_stride < value_size`, a NULL required pointer (`pe`, `dpe`, the workspace; every other array when `n_rows > 0`):
 *   SE3_ERR_INVALID_ARGUMENT;
 * - `num_basis > SE3_BASIS_ATT_MAX_BASIS`, or one of `N * 2V * K`, `N * K * H`, `N * key_stride`, `K * V` at or beyond `2^31`:
 *   SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_BASIS_ATT_H_
#define SE3CONV_BASIS_ATT_H_

#include <stddef.h>
#include <stdint.h>

/* points per chunk of the order of additions of `dpe`: a multiple of 64.  Part of the arithmetic contract
 * (tests/basis_att_reference.py holds the same number). */
#define SE3_BASIS_ATT_CHUNK 256
/* the most basis functions the softmax runs over (se3_feat_basis_proj takes 8, 16, 32 and 64) */
#define SE3_BASIS_ATT_MAX_BASIS 64

#ifdef __cplusplus
extern "C" {
#endif

/* host only */
size_t se3_basis_att_workspace_bytes(int64_t n_rows, int32_t value_size, int32_t num_heads, int32_t num_basis);

int se3_basis_att_fwd(const float* T, const float* key, int64_t key_stride, const float* pe, int64_t n_rows,
                      int32_t value_size, int32_t num_heads, int32_t num_basis, float* att, float* out, void* stream);

int se3_basis_att_bwd(const float* grad_out, const float* T, const float* key, int64_t key_stride, const float* pe,
                      const float* att, int64_t n_rows, int32_t value_size, int32_t num_heads, int32_t num_basis,
                      float* dT, float* dkey, float* dpe, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_BASIS_ATT_H_ */
