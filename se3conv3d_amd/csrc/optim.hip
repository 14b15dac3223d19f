// Optimizer step (include/se3conv_optim.h): the global gradient norm in a fixed fp64 order, the clip coefficient, the AdamW
// update, the schedule's learning rate and the accumulation gate, with the counters in device words.  Three kernels:
//
//   partials  grid-stride over the chunk table on resident workgroups of 256 threads.  Lane j squares elements 4j .. 4j+3 of
//             the chunk in fp64 (exact), adds them as the header pairs them, and the workgroup runs the header's tree over 256
//             fp64 words of LDS.  One fp64 partial per chunk goes to the workspace.
//   finish    ONE workgroup: lane j adds the partials j, j + 256, ... in ascending order, the same tree gives the total, and
//             lane 0 computes every scalar of the call -- norm, coefficient, learning rate, gate, bias corrections -- updates
//             the state words, writes the read-out words and leaves the update's orders in the workspace.  All of lane 0's
//             words go out with ordinary (vector) stores.
//   update    grid-stride over the chunk table again: reads the orders, and either leaves at once (a gated call: no byte is
//             written), zeroes the gradients (a skipped step), or runs the header's per-element sequence.
//
// A chunk takes the 16-byte form when its tensor's parameter and gradient addresses are 16-byte aligned (the chunk offset,
// 1024 elements, and the state offset, a multiple of 4 from an aligned base, keep that), the 4-byte form elsewhere: uniform in
// the workgroup.  In both forms lane j owns elements 4j .. 4j+3, so the arithmetic and its order are the same; a lane whose
// four elements are not all in front of `numel` falls back to 4-byte accesses of those that are, so nothing behind `numel` is
// touched.  The per-element sequence stands in a function under `fp contract(off)`: `/` and `sqrtf` are then IEEE operations
// (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), denormals are kept (the default float mode of a kernel).
#include <math.h>

#include "common.h"
#include "../../include/se3conv_optim.h"

namespace se3 {
namespace {

constexpr int kChunk = SE3_OPTIM_CHUNK;
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8 resident workgroups; the rest of the table is grid-strided
static_assert(kChunk == 4 * kThreads, "one lane per four elements of a chunk");

// what `finish` leaves for `update`
struct Orders {
  int32_t mode;  // 0: nothing (a gated call), 1: update, 2: zero the gradients only (a skipped step)
  float clip_coef, lr, step_size, bc2s;
};
enum { kModeNone = 0, kModeUpdate = 1, kModeZero = 2 };

struct OptimLayout {
  size_t partials, orders, total;
};

OptimLayout optim_layout(int64_t n_chunks) {
  OptimLayout l{};
  l.partials = 0;
  l.orders = align_up((size_t)(n_chunks > 0 ? n_chunks : 1) * sizeof(double), 256);
  l.total = l.orders + 256;
  return l;
}

struct StepConsts {  // host-computed, by value
  double beta1, beta2;
  float w1, w2, b2f, epsf, max_norm;
  int32_t accum, zero_grads, skip_nonfinite;
  int64_t n_lr;
};

__device__ __forceinline__ bool aligned16_dev(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the header's tree over 256 fp64 words: afterwards s[0] holds the sum (every lane calls this)
__device__ __forceinline__ double tree256(double* s, double mine) {
  const int j = threadIdx.x;
  s[j] = mine;
  __syncthreads();
#pragma unroll
  for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
    if (j < stride) s[j] = s[j] + s[j + stride];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();  // (the next chunk overwrites s)
  return r;
}

__device__ __forceinline__ double sq4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const double a2 = (double)a * (double)a, b2 = (double)b * (double)b, c2 = (double)c * (double)c, d2 = (double)d * (double)d;
  return (a2 + b2) + (c2 + d2);
}

__global__ __launch_bounds__(kThreads) void optim_partials_kernel(const se3_optim_tensor* __restrict__ tensors,
                                                                  const se3_optim_chunk* __restrict__ chunks, int n_chunks,
                                                                  double* __restrict__ partials) {
  __shared__ double s[kThreads];
  const int j = threadIdx.x, base = 4 * j;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const se3_optim_chunk ck = chunks[c];
    const se3_optim_tensor tn = tensors[ck.tensor];
    const int64_t e0 = (int64_t)ck.index * kChunk;
    const int n = (int)min((int64_t)kChunk, tn.numel - e0);
    const float* g = tn.grad + e0;
    float x[4] = {0.f, 0.f, 0.f, 0.f};  // an element the chunk does not have: +0.0
    if (aligned16_dev(tn.grad) && base + 3 < n) {
      const float4 q = *reinterpret_cast<const float4*>(g + base);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (base + k < n) x[k] = g[base + k];
    }
    const double total = tree256(s, sq4(x[0], x[1], x[2], x[3]));
    if (j == 0) partials[c] = total;
  }
}

// the total of `n` partials in the header's order (every lane of the one workgroup calls this)
__device__ __forceinline__ double total_of(const double* __restrict__ partials, int64_t n, double* s) {
#pragma clang fp contract(off)
  double u = 0.0;
  for (int64_t c = threadIdx.x; c < n; c += kThreads) u = u + partials[c];
  return tree256(s, u);
}

__global__ __launch_bounds__(kThreads) void optim_norm_finish_kernel(const double* __restrict__ partials, int64_t n_chunks,
                                                                     float* __restrict__ grad_norm) {
  __shared__ double s[kThreads];
  const double total = total_of(partials, n_chunks, s);
  if (threadIdx.x == 0) *grad_norm = (float)sqrt(total);
}

__device__ __forceinline__ float clip_coefficient(float max_norm, float grad_norm) {
#pragma clang fp contract(off)
  const float den = grad_norm + 1e-6f;
  const float c = max_norm / den;
  return c > 1.0f ? 1.0f : c;  // a NaN stays a NaN
}

__global__ __launch_bounds__(kThreads) void optim_step_finish_kernel(const double* __restrict__ partials, int64_t n_norm_chunks,
                                                                     int want_norm, const float* __restrict__ lr_table,
                                                                     StepConsts k, int64_t* state, void* readout,
                                                                     Orders* __restrict__ orders) {
#pragma clang fp contract(off)
  __shared__ double s[kThreads];
  double total = 0.0;
  if (want_norm) total = total_of(partials, n_norm_chunks, s);  // (uniform)
  if (threadIdx.x != 0) return;
  const float grad_norm = want_norm ? (float)sqrt(total) : 0.0f;
  int64_t it = state[0], t = state[1], skipped = state[4];
  double b1p = __builtin_bit_cast(double, state[2]), b2p = __builtin_bit_cast(double, state[3]);
  const bool gate = (it % (int64_t)k.accum) == 0;
  const int64_t at = it < 0 ? 0 : (it < k.n_lr - 1 ? it : k.n_lr - 1);
  const float lr = lr_table[at];
  const bool clip = k.max_norm > 0.0f;
  const float coef = clip ? clip_coefficient(k.max_norm, grad_norm) : 1.0f;
  Orders o{kModeNone, coef, lr, 0.0f, 1.0f};
  int32_t stepped = 0;
  if (gate) {
    if (k.skip_nonfinite && !isfinite(grad_norm)) {
      skipped += 1;
      o.mode = k.zero_grads ? kModeZero : kModeNone;
    } else {
      t += 1;
      b1p = b1p * k.beta1;
      b2p = b2p * k.beta2;
      const double bc1 = 1.0 - b1p, bc2 = 1.0 - b2p;
      o.step_size = (float)((double)lr / bc1);
      o.bc2s = (float)sqrt(bc2);
      o.mode = kModeUpdate;
      stepped = 1;
    }
  }
  it += 1;
  state[0] = it, state[1] = t, state[4] = skipped;
  state[2] = __builtin_bit_cast(int64_t, b1p), state[3] = __builtin_bit_cast(int64_t, b2p);
  float* rf = reinterpret_cast<float*>(readout);
  rf[0] = grad_norm, rf[1] = coef, rf[2] = lr;
  reinterpret_cast<int32_t*>(readout)[3] = stepped;
  *orders = o;
}

struct ElemConsts {
  float coef, factor, w1, w2, b2f, epsf, step_size, bc2s;
  bool clip;
};

// one element, as the header states it: every line one fp32 operation, rounded once
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const ElemConsts& c) {
#pragma clang fp contract(off)
  if (c.clip) g = g * c.coef;
  const float p1 = p * c.factor;
  const float dm = g - m;
  const float dmw = dm * c.w1;
  const float m1 = m + dmw;
  const float vb = v * c.b2f;
  const float gg = g * g;
  const float ggw = gg * c.w2;
  const float v1 = vb + ggw;
  const float r = sqrtf(v1);
  const float rb = r / c.bc2s;
  const float d = rb + c.epsf;
  const float q = m1 / d;
  const float sq = c.step_size * q;
  p = p1 - sq;
  m = m1, v = v1;
}

__device__ __forceinline__ float decay_factor(float lr, float decay) {
#pragma clang fp contract(off)
  const double ld = (double)lr * (double)decay;
  return (float)(1.0 - ld);
}

__global__ __launch_bounds__(kThreads) void optim_update_kernel(const se3_optim_tensor* __restrict__ tensors,
                                                                const se3_optim_chunk* __restrict__ chunks, int n_chunks,
                                                                const float* __restrict__ decay, float* __restrict__ exp_avg,
                                                                float* __restrict__ exp_avg_sq,
                                                                const Orders* __restrict__ orders, StepConsts k) {
  const Orders o = *orders;
  if (o.mode == kModeNone) return;  // (the whole grid) a gated call writes no byte
  const int j = threadIdx.x, base = 4 * j;
  const bool zero = k.zero_grads != 0;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const se3_optim_chunk ck = chunks[c];
    const se3_optim_tensor tn = tensors[ck.tensor];
    const int64_t e0 = (int64_t)ck.index * kChunk;
    const int n = (int)min((int64_t)kChunk, tn.numel - e0);
    float* g = tn.grad + e0;
    const bool vec = aligned16_dev(tn.param) && aligned16_dev(tn.grad) && base + 3 < n;
    if (o.mode == kModeZero) {
      if (vec) {
        *reinterpret_cast<float4*>(g + base) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (base + e < n) g[base + e] = 0.f;
      }
      continue;
    }
    float* p = tn.param + e0;
    float* m = exp_avg + tn.state_offset + e0;
    float* v = exp_avg_sq + tn.state_offset + e0;
    const ElemConsts ec{o.clip_coef, decay_factor(o.lr, decay[ck.tensor]), k.w1, k.w2, k.b2f, k.epsf, o.step_size, o.bc2s,
                        k.max_norm > 0.0f};
    if (vec) {
      float4 pp = *reinterpret_cast<const float4*>(p + base);
      const float4 gq = *reinterpret_cast<const float4*>(g + base);
      float4 mm = *reinterpret_cast<const float4*>(m + base);
      float4 vv = *reinterpret_cast<const float4*>(v + base);
      adamw_element(pp.x, gq.x, mm.x, vv.x, ec);
      adamw_element(pp.y, gq.y, mm.y, vv.y, ec);
      adamw_element(pp.z, gq.z, mm.z, vv.z, ec);
      adamw_element(pp.w, gq.w, mm.w, vv.w, ec);
      *reinterpret_cast<float4*>(p + base) = pp;
      *reinterpret_cast<float4*>(m + base) = mm;
      *reinterpret_cast<float4*>(v + base) = vv;
      if (zero) *reinterpret_cast<float4*>(g + base) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = base + e;
        if (i < n) {
          float pe = p[i], me = m[i], ve = v[i];
          adamw_element(pe, g[i], me, ve, ec);
          p[i] = pe, m[i] = me, v[i] = ve;
          if (zero) g[i] = 0.f;
        }
      }
    }
  }
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the checks of the tables both device calls share
int optim_tables(const void* tensors, int32_t n_tensors, const void* chunks, int64_t n_chunks, const void* workspace,
                 size_t workspace_bytes) {
  if (n_tensors < 0 || n_chunks < 0) return SE3_ERR_INVALID_ARGUMENT;
  if (n_chunks >= (1ll << 31)) return SE3_ERR_UNSUPPORTED;
  if ((n_tensors > 0 && !tensors) || (n_chunks > 0 && (!chunks || n_tensors == 0)) || !workspace) return SE3_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < optim_layout(n_chunks).total) return SE3_ERR_WORKSPACE;
  return SE3_OK;
}

unsigned grid_of(int64_t n_chunks) { return (unsigned)(n_chunks < kMaxBlocks ? n_chunks : kMaxBlocks); }

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" int se3_optim_plan(const int64_t* numel, int32_t n_tensors, struct se3_optim_tensor* tensors_out,
                              struct se3_optim_chunk* chunks_out, int64_t chunk_capacity, int64_t* n_chunks, int64_t* state_len) {
  if (n_tensors < 0 || (n_tensors > 0 && !numel) || !n_chunks || !state_len || (chunks_out && chunk_capacity < 0))
    return SE3_ERR_INVALID_ARGUMENT;
  int64_t chunks = 0, len = 0;
  for (int32_t t = 0; t < n_tensors; ++t) {
    if (numel[t] < 0 || numel[t] > (1ll << 46)) return SE3_ERR_INVALID_ARGUMENT;
    chunks += (numel[t] + kChunk - 1) / kChunk;
    len += (numel[t] + 3) / 4 * 4;
  }
  if (chunks >= (1ll << 31)) return SE3_ERR_UNSUPPORTED;
  if (chunks_out && chunk_capacity < chunks) return SE3_ERR_INVALID_ARGUMENT;
  int64_t c = 0, off = 0;
  for (int32_t t = 0; t < n_tensors; ++t) {
    const int64_t own = (numel[t] + kChunk - 1) / kChunk;
    if (tensors_out) tensors_out[t].numel = numel[t], tensors_out[t].state_offset = off;
    if (chunks_out)
      for (int64_t i = 0; i < own; ++i) chunks_out[c + i] = se3_optim_chunk{t, (int32_t)i};
    c += own;
    off += (numel[t] + 3) / 4 * 4;
  }
  *n_chunks = chunks, *state_len = len;
  return SE3_OK;
}

extern "C" size_t se3_optim_workspace_bytes(int64_t n_chunks) {
  if (n_chunks < 0 || n_chunks >= (1ll << 31)) return 0;
  return optim_layout(n_chunks).total;
}

extern "C" int se3_optim_grad_norm(const struct se3_optim_tensor* tensors, int32_t n_tensors, const struct se3_optim_chunk* chunks,
                                   int64_t n_chunks, float* grad_norm, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = optim_tables(tensors, n_tensors, chunks, n_chunks, workspace, workspace_bytes)) return rc;
  if (!grad_norm) return SE3_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  double* partials = (double*)((char*)workspace + optim_layout(n_chunks).partials);
  if (n_chunks > 0)
    hipLaunchKernelGGL(optim_partials_kernel, dim3(grid_of(n_chunks)), dim3(kThreads), 0, stream, tensors, chunks, (int)n_chunks,
                       partials);
  hipLaunchKernelGGL(optim_norm_finish_kernel, dim3(1), dim3(kThreads), 0, stream, partials, n_chunks, grad_norm);
  return check_launch();
}

extern "C" int se3_optim_adamw_step(const struct se3_optim_tensor* tensors, int32_t n_tensors, const struct se3_optim_chunk* chunks,
                                    int64_t n_chunks, const float* decay, float* exp_avg, float* exp_avg_sq, void* state,
                                    void* readout, const float* lr_table, int64_t n_lr, double beta1, double beta2, double eps,
                                    float max_norm, int32_t accum, int32_t zero_grads, int32_t skip_nonfinite, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
  if (n_lr < 1 || accum < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
    return SE3_ERR_INVALID_ARGUMENT;
  if (int rc = optim_tables(tensors, n_tensors, chunks, n_chunks, workspace, workspace_bytes)) return rc;
  if (!state || !readout || !lr_table || (n_tensors > 0 && !decay) || (n_chunks > 0 && (!exp_avg || !exp_avg_sq)))
    return SE3_ERR_INVALID_ARGUMENT;
  if (!aligned_to(exp_avg, 16) || !aligned_to(exp_avg_sq, 16) || !aligned_to(state, 8) || !aligned_to(readout, 4))
    return SE3_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const OptimLayout l = optim_layout(n_chunks);
  double* partials = (double*)((char*)workspace + l.partials);
  Orders* orders = (Orders*)((char*)workspace + l.orders);
  const StepConsts k{beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)beta2, (float)eps, max_norm,
                     accum, zero_grads, skip_nonfinite, n_lr};
  const bool want_norm = max_norm > 0.0f || skip_nonfinite != 0;
  if (want_norm && n_chunks > 0)
    hipLaunchKernelGGL(optim_partials_kernel, dim3(grid_of(n_chunks)), dim3(kThreads), 0, stream, tensors, chunks, (int)n_chunks,
                       partials);
  hipLaunchKernelGGL(optim_step_finish_kernel, dim3(1), dim3(kThreads), 0, stream, partials, n_chunks, (int)want_norm, lr_table, k,
                     (int64_t*)state, readout, orders);
  if (n_chunks > 0)
    hipLaunchKernelGGL(optim_update_kernel, dim3(grid_of(n_chunks)), dim3(kThreads), 0, stream, tensors, chunks, (int)n_chunks, decay,
                       exp_avg, exp_avg_sq, orders, k);
  return check_launch();
}
