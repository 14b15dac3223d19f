/*
 * se3conv_pne.h -- the point-neighbourhood embeddings of libse3conv_hip.so besides the fused operator's own (the reference's
 * `LinearPNE` with its five activations and `KPPNE` with its three correlation functions), and the max aggregation of the
 * non-equivariant layer (`TransformNeighConv` + `scatter_max`) in a form that never builds an `E x C_in x C_out` tensor.
 *
 * Same conventions as se3conv_global_pool.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, no
 * atomics, int status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * Shapes
 * - `neighbors [E,2]` int32, `(sample, source)` per edge, grouped by sample in ascending sample order; `ends [M]` int32,
 *   inclusive end offsets: the edges of sample `m` are `[ends[m-1], ends[m])` with `ends[-1] = 0`.  Every one of the `E` rows
 *   is an edge (capacity-bounded buffers are not taken).
 * - `pts [N,3]`, `samples [M,3]` fp32; `rho` one fp32 word on the device; `K = num_basis >= 1`.
 * - Every byte of every output is written; nothing depends on what the outputs or the workspace held before.  `E == 0` is valid.
 *
 * The arithmetic, normatively (tests/pne_reference.py restates it in float64 numpy).  "fp32" operations are IEEE operations
 * rounded to nearest even; `fma(a, b, c)` is the fused operation, one rounding.  erf, exp, sin, cos and sqrt are the
 * device's fp32 library functions.
 *
 * se3_pne_embed_fwd -- `phi [E,K]`
 * - `r[d] = (pts[src, d] - samples[smp, d]) * rho`, a subtraction, then a product.
 * - The inputs `in[0 .. J')` of the projection:
 *   - MLP kinds: `J' = 3`, `in = r`, `A [3,K]`.
 *   - kernel-point kinds: `J' = J = n_kpts` (`1 <= J <= SE3_PNE_MAX_KPTS`), `kpts [J,3]`, `A [J,K]`.  With `u[d] = r[d] - kpts[j,d]`,
 *     `d2[j] = fma(u[2], u[2], fma(u[1], u[1], u[0] * u[0]))` and `t[j] = sqrt(d2[j]) / sigma`:
 *       SE3_PNE_KP_GAUSS   `in[j] = exp(-(t * t) * 0.5f)`
 *       SE3_PNE_KP_LINEAR  `in[j] = max(1 - t, 0)`
 *       SE3_PNE_KP_BOX     `in[j] = 1` for the `j` of the smallest `d2[j]`, the LOWEST such `j` on a tie, `0` for the others.
 * - `z[k] = beta[k]`, then `z[k] = fma(in[j], A[j,k], z[k])` in ascending `j`.
 * - `phi[k] = act(z[k])`: the kernel-point kinds and SE3_PNE_MLP_LINEAR `z`; RELU `max(z, 0)`; GELU `0.5 z (1 + erf(z / sqrt 2))`
 *   (the exact form, `torch.nn.GELU()`); SIN `sin(z)`; SOFTMAX `e[k] / s` with `m = max_k z[k]`, `e[k] = exp(z[k] - m)` and
 *   `s` the fp32 sum of `e[k]` in ascending `k`, starting from `+0.0f`.
 *
 * se3_pne_embed_bwd -- `dA [J',K]`, `dbeta [K]` from `grad_phi [E,K]`; there is no gradient to points, as in the reference
 * - `in`, `z` and `phi` are recomputed as above.  `gz[k]`, in fp32: kernel-point kinds and LINEAR `g[k]`; RELU `z > 0 ? g : 0`;
 *   GELU `g * (0.5 (1 + erf(z / sqrt 2)) + z exp(-z z / 2) / sqrt(2 pi))`; SIN `g * cos(z)`; SOFTMAX `phi[k] * (g[k] - q)` with
 *   `q` the fp32 sum `fma(g[k], phi[k], q)` in ascending `k`, starting from `+0.0f`.
 * - Chunk `c` covers the edges `[c * SE3_PNE_CHUNK, (c + 1) * SE3_PNE_CHUNK)`.  The partials of `(c, j, k)` start at `+0.0` and
 *   add, as fp64 and in ascending edge order, `(double)in[j] * (double)gz[k]` (exact) for `dA` and `(double)gz[k]` for `dbeta`.
 *   The totals start at `+0.0` and add the partials in ascending `c`; stored as float.  Two calls give the same bits.
 *
 * se3_neigh_max_fwd -- `out [M,C_out]`, `arg [M,C_out]` from `phi [E,K]` and `G [N,K,C_out]`, the source features already
 * multiplied by the conv weights (`G = feat @ W.reshape(C_in, K * C_out)`); `C_out >= 1`
 * - Per edge `v[o] = +0.0f`, then `v[o] = fma(phi[e,k], G[src,k,o], v[o])` in ascending `k`.
 * - `out[m,o]` is the largest `v[o]` over the edges of `m`, `arg[m,o]` the index of that edge (a row of `neighbors`): the
 *   first edge is taken, a later one replaces it when its `v` is GREATER (`>`), so a tie keeps the lowest edge index.
 * - A sample without edges gets `out = +0.0f`, `arg = -1`: always `M` rows.
 *
 * se3_neigh_max_bwd -- `dphi [E,K]`, `dG [N,K,C_out]` from `grad_out [M,C_out]` and `arg` as the forward call wrote it
 * - `dphi[e,k]` starts at `+0.0f` and adds `fma(grad_out[m,o], G[src,k,o], .)` over the `o` with `arg[m,o] == e`, ascending.
 * - `dG[p,k,o]` starts at `+0.0f` and adds `fma(grad_out[m,o], phi[e,k], .)` over the incoming edges `e = (m, p)` of source
 *   `p` with `arg[m,o] == e`, in the order of `t_samples [E]`, `t_ends [N]`, `t_edge_ids [E]` -- the source-major
 *   transposition of `neighbors` that se3_csr_transpose writes (ascending edge index within a source).  No atomic: a row of
 *   `dphi` belongs to one sample and a row of `dG` to one source.  Rows that win nowhere are `+0.0f`.
 *
 * Workspace: `se3_pne_embed_workspace_bytes(n_edges, kind, n_kpts, num_basis)` bytes serve se3_pne_embed_bwd -- 8 bytes per
 * (chunk, input or bias, basis function); 0 for arguments the calls refuse.  The other calls need none.
 *
 * Errors, all checked on the host before the first launch
 * - a negative count, `num_basis < 1`, `c_out < 1`, a `kind` outside the enum, a kernel-point kind with `n_kpts < 1`, `kpts == NULL`
 *   or a `sigma` that is not a positive finite number, a NULL required pointer (`rho`, `A`, `beta`, `dA`, `dbeta`, the workspace;
 *   every other array when it has a row): SE3_ERR_INVALID_ARGUMENT;
 * - `n_kpts > SE3_PNE_MAX_KPTS`, or one of `E * K`, `E * 2`, `N * K * C_out`, `M * C_out`, `J' * K` at or beyond `2^31`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 */
#ifndef SE3CONV_PNE_H_
#define SE3CONV_PNE_H_

#include <stddef.h>
#include <stdint.h>

/* edges per chunk of the order of additions of se3_pne_embed_bwd: a multiple of 64.  Part of the arithmetic contract
 * (tests/pne_reference.py holds the same number). */
#define SE3_PNE_CHUNK 1024
/* the most kernel points a kernel-point embedding takes (the reference's sets have 13 and 55) */
#define SE3_PNE_MAX_KPTS 64

enum se3_pne_kind {
  SE3_PNE_MLP_LINEAR = 0,
  SE3_PNE_MLP_RELU = 1,
  SE3_PNE_MLP_GELU = 2,
  SE3_PNE_MLP_SIN = 3,
  SE3_PNE_MLP_SOFTMAX = 4,
  SE3_PNE_KP_GAUSS = 5,
  SE3_PNE_KP_LINEAR = 6,
  SE3_PNE_KP_BOX = 7
};

#ifdef __cplusplus
extern "C" {
#endif

/* host only */
size_t se3_pne_embed_workspace_bytes(int64_t n_edges, int32_t kind, int32_t n_kpts, int32_t num_basis);

int se3_pne_embed_fwd(const float* pts, const float* samples, const int32_t* neighbors, int64_t n_edges, const float* rho,
                      int32_t kind, const float* kpts, int32_t n_kpts, float sigma, const float* A, const float* beta,
                      int32_t num_basis, float* phi, void* stream);

int se3_pne_embed_bwd(const float* grad_phi, const float* pts, const float* samples, const int32_t* neighbors, int64_t n_edges,
                      const float* rho, int32_t kind, const float* kpts, int32_t n_kpts, float sigma, const float* A,
                      const float* beta, int32_t num_basis, float* dA, float* dbeta, void* workspace, size_t workspace_bytes,
                      void* stream);

int se3_neigh_max_fwd(const float* phi, const float* G, const int32_t* neighbors, const int32_t* ends, int64_t n_edges,
                      int64_t n_samples, int64_t n_src, int32_t num_basis, int32_t c_out, float* out, int32_t* arg, void* stream);

int se3_neigh_max_bwd(const float* grad_out, const int32_t* arg, const float* phi, const float* G, const int32_t* neighbors,
                      const int32_t* ends, const int32_t* t_samples, const int32_t* t_ends, const int32_t* t_edge_ids,
                      int64_t n_edges, int64_t n_samples, int64_t n_src, int32_t num_basis, int32_t c_out, float* dphi, float* dG,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_PNE_H_ */
