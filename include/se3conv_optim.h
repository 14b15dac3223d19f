/*
 * se3conv_optim.h -- the optimizer step of libse3conv_hip.so: the global L2 norm of all gradients, the clip coefficient, one
 * AdamW update of every parameter, the learning rate of a schedule table and the gradient-accumulation gate, with every
 * counter in device words, without an atomic on a float or on global memory and in a fixed order of additions: two runs of a
 * training job give the same bits, and the call is capturable.  It replaces, inside a captured step, the last three lines of
 * the reference's training loops (tasks/SemSeg/train_*_rot.py, tasks/Classification/train_rot.py): `clip_grad_norm_`,
 * `optim.step(); optim.zero_grad()` under the Python `if cur_iter % accum_grads == 0`, and `scheduler.step()`.
 *
 * Same conventions as se3conv_seg_head.h (extern "C", device pointers unless marked "host", caller-owned outputs and
 * workspace, asynchronous on `stream`, no host synchronisation, no stream, event or allocation created, no memset calls, int
 * status; every error is checked on the host before the first launch).  These entry points are additions inside
 * SE3_ABI_VERSION 6: se3conv.h and its version number are unchanged.
 *
 * The parameter set: `n_tensors` fp32 tensors of any sizes, described once by device tables that the caller builds and keeps
 * - `tensors [n_tensors]` of `struct se3_optim_tensor`: the parameter address, the gradient address, `numel`, and
 *   `state_offset`, the element offset of the tensor into the two flat fp32 state buffers `exp_avg` and `exp_avg_sq`.
 *   Offsets are multiples of 4 and ascend; the state bases are 16-byte aligned, so a tensor's state is always 16-byte aligned.
 * - `chunks [n_chunks]` of `struct se3_optim_chunk`: a chunk is SE3_OPTIM_CHUNK (1024) consecutive elements of ONE tensor,
 *   `{tensor, index}` = elements `[index * 1024, min((index + 1) * 1024, numel))` of `tensors[tensor]`.  Tensor `t` owns
 *   `ceil(numel_t / 1024)` chunks (none when `numel_t == 0`); tensors ascend, and chunks ascend inside a tensor.  No chunk
 *   straddles two tensors.
 * - `decay [n_tensors]` fp32: the weight decay of each tensor.
 * `se3_optim_plan` (host only) fills the host images of the two tables from the `numel`s: `numel` and `state_offset` of every
 * tensor (`param` and `grad` are left as they are: the caller's), every chunk, `*n_chunks` and `*state_len` (the length of
 * each state buffer in elements, the sum of the `numel`s each rounded up to 4).  `tensors_out` and `chunks_out` may be NULL (a
 * counting call); `chunk_capacity` is the room of `chunks_out` in chunks.  `se3_optim_workspace_bytes(n_chunks)` (host only)
 * is the workspace both device calls need: one fp64 partial per chunk and the words the finishing launch hands the update;
 * 0 for an `n_chunks` the calls refuse.
 *
 * Device words
 * - `state`: SE3_OPTIM_STATE_WORDS (5) 8-byte words that persist across calls and are what a checkpoint stores:
 *   `[0] it` calls so far (int64), `[1] t` updates taken (int64), `[2] b1p = beta1^t`, `[3] b2p = beta2^t` (fp64, kept as
 *   running products: no `pow`), `[4] skipped` (int64).  A fresh optimizer holds `{0, 0, 1.0, 1.0, 0}`.
 * - `readout`: SE3_OPTIM_READOUT_WORDS (4) 4-byte words written by every call of se3_optim_adamw_step:
 *   `[0] grad_norm`, `[1] clip_coef`, `[2] lr` (fp32), `[3] stepped` (int32).
 *
 * se3_optim_grad_norm: `*grad_norm` = the global L2 norm of all gradients, in this order (tests/optim_reference.py restates it)
 * - The square of an element is `(double)x * (double)x`, which is exact.
 * - Chunk partial, with the elements a chunk does not have (behind `numel`) as `+0.0`:
 *   `s_j = (x2[4j] + x2[4j+1]) + (x2[4j+2] + x2[4j+3])` for `j = 0..255`, then one pairwise tree
 *   `s_j += s_{j+stride}` for `stride = 128, 64, ..., 1` (`j < stride`); the partial is `s_0`.
 * - Total over chunks `c = 0 .. n_chunks - 1`: `u_j` = the sum of the partials `j, j + 256, j + 512, ...` ascending, starting
 *   from `+0.0`, for `j = 0..255`; then the same tree over `u`; the total is `u_0`.
 * - `grad_norm = (float)sqrt(total)`, the fp64 square root correctly rounded.
 * The order is a function of the tables alone: not of the grid, of an address's alignment or of the kernel form.
 *
 * se3_optim_adamw_step.  Scalar arguments: `beta1`, `beta2`, `eps` (double, by value), `max_norm` (fp32; `<= 0` or NaN: no
 * clipping), `accum` (>= 1), `lr_table [n_lr]` (fp32, on the device), the flags `zero_grads` and `skip_nonfinite`.
 * The norm pass runs iff `max_norm > 0` or `skip_nonfinite`; without it `grad_norm = 0.0f`.  One thread computes the scalars:
 * - `do = (it % accum == 0)`                (the `it` of BEFORE the call: with `accum = 3` the calls 0, 3, 6, ... update)
 * - `lr = lr_table[min(it, n_lr - 1)]`
 * - `c = max_norm / (grad_norm + 1e-6f)` in fp32, `clip_coef = c > 1.0f ? 1.0f : c` (a NaN stays a NaN, as in torch);
 *   `clip_coef = 1.0f` without clipping.
 * - with `skip_nonfinite` and a `grad_norm` that is not finite, on a call with `do`: `skipped += 1`, `stepped = 0`, and `p`,
 *   `m`, `v`, `t`, `b1p`, `b2p` stay as they are; the gradients are zeroed when `zero_grads`.
 * - else when `do`: `t += 1`, `b1p *= beta1`, `b2p *= beta2`, `step_size = (float)((double)lr / (1 - b1p))`,
 *   `bc2s = (float)sqrt(1 - b2p)`, `w1 = (float)(1 - beta1)`, `w2 = (float)(1 - beta2)`, `b2f = (float)beta2`,
 *   `epsf = (float)eps`, `stepped = 1`.
 * - `it += 1`, always: the reference steps its scheduler every iteration.
 * Per element when updating, every operation a single fp32 operation rounded once to nearest even -- no contraction, denormals
 * kept, divide and square root correctly rounded (`m`, `v`: the element of `exp_avg`, `exp_avg_sq`):
 *     g  = grad * clip_coef                              (only when max_norm > 0)
 *     p1 = p * (float)(1.0 - (double)lr * (double)decay_t)
 *     m' = m + (g - m) * w1
 *     v' = (v * b2f) + ((g * g) * w2)
 *     d  = sqrtf(v') / bc2s + epsf
 *     p' = p1 - step_size * (m' / d)
 *     grad = +0.0f                                       (when zero_grads)
 * which is the single-tensor path of torch.optim.AdamW with its operations named.  When not `do`, no byte of `p`, `m`, `v` or
 * `grad` is written and `stepped = 0`.  Nothing behind `numel` of any tensor is read or written, whichever kernel form runs:
 * 16-byte accesses where a tensor's parameter and gradient addresses are 16-byte aligned, 4-byte accesses elsewhere, the same
 * bits from both.
 *
 * Launches: chunk partials (only with the norm pass), one finishing workgroup that also writes the words, the update -- at
 * most three per call, and the same ones on every call with the same arguments: a captured graph replays them.
 *
 * Errors, all checked on the host before the first launch
 * - a NULL required pointer (`state`, `readout`, `lr_table`, the workspace; the tables and `decay` when `n_tensors > 0`, the
 *   chunk table when `n_chunks > 0`, the state buffers when `n_chunks > 0`; `grad_norm` of se3_optim_grad_norm), a negative
 *   count, `accum < 1`, `n_lr < 1`, a `beta` outside `[0, 1)` or NaN, a negative or NaN `eps`, a state base that is not
 *   16-byte aligned: SE3_ERR_INVALID_ARGUMENT;
 * - `n_chunks >= 2^31`: SE3_ERR_UNSUPPORTED;
 * - `workspace_bytes` below the query's value: SE3_ERR_WORKSPACE.
 * `n_tensors == 0`, `n_chunks == 0` and tensors of `numel == 0` are valid: the words still advance.
 */
#ifndef SE3CONV_OPTIM_H_
#define SE3CONV_OPTIM_H_

#include <stddef.h>
#include <stdint.h>

#define SE3_OPTIM_CHUNK 1024        /* elements per chunk: part of the arithmetic contract of the norm */
#define SE3_OPTIM_STATE_WORDS 5     /* 8-byte words of `state` */
#define SE3_OPTIM_READOUT_WORDS 4   /* 4-byte words of `readout` */

#ifdef __cplusplus
extern "C" {
#endif

struct se3_optim_tensor {
  float* param;           /* [numel] fp32, device */
  float* grad;            /* [numel] fp32, device */
  int64_t numel;
  int64_t state_offset;   /* elements into exp_avg / exp_avg_sq: a multiple of 4 */
};

struct se3_optim_chunk {
  int32_t tensor;         /* index into the tensor table */
  int32_t index;          /* which chunk of that tensor */
};

/* host only: every pointer is a host pointer */
int se3_optim_plan(const int64_t* numel, int32_t n_tensors, struct se3_optim_tensor* tensors_out,
                   struct se3_optim_chunk* chunks_out, int64_t chunk_capacity, int64_t* n_chunks, int64_t* state_len);

/* host only */
size_t se3_optim_workspace_bytes(int64_t n_chunks);

int se3_optim_grad_norm(const struct se3_optim_tensor* tensors, int32_t n_tensors, const struct se3_optim_chunk* chunks,
                        int64_t n_chunks, float* grad_norm, void* workspace, size_t workspace_bytes, void* stream);

int se3_optim_adamw_step(const struct se3_optim_tensor* tensors, int32_t n_tensors, const struct se3_optim_chunk* chunks,
                         int64_t n_chunks, const float* decay, float* exp_avg, float* exp_avg_sq, void* state, void* readout,
                         const float* lr_table, int64_t n_lr, double beta1, double beta2, double eps, float max_norm,
                         int32_t accum, int32_t zero_grads, int32_t skip_nonfinite, void* workspace, size_t workspace_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SE3CONV_OPTIM_H_ */
