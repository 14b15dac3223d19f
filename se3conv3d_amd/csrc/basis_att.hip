// Softmax attention over the basis functions of an aggregated [N, 2V, K] tensor (include/se3conv_basis_att.h).
//
//   fwd / bwd   everything of a (point, head) pair is independent of every other pair, so a GROUP of lanes takes one pair: the
//               lanes of a group run along k (four consecutive k per lane and 16-byte accesses where K % 4 == 0 and the tensors
//               are 16-byte aligned, one k per lane otherwise), a group has the next power of two of lanes, groups fill the
//               wavefronts in (point, head) order, and a group walks the D channels of its head, kAhead rows in flight.  Adjacent
//               groups read adjacent K * D * 4-byte pieces of T, every piece whole.  The sums over the channels of a head
//               (s, datt) are fma chains in a lane's registers; the sums over k (softmax denominator, out, dkey, the softmax
//               backward's mean) are the pairwise tree of the header: inside a lane, then xor shuffles over the group.  Every
//               element of T is loaded once: Tq for s, Tv for out (fwd); Tv for datt, Tq for dkey (bwd).  Nothing goes through
//               LDS but `pe`, whose [K,V] layout is the transpose of what the lanes need: a workgroup stages it once, as
//               pe_s[i][k] with an odd row length, for the kIters batches of groups it walks (a `pe` beyond kPeLdsFloats is
//               read from memory instead: the same values, slower).
//   dpe         dpe[k,i] is the sum over the points of dTq[i,k], which the backward kernel has just written: a workgroup takes
//               a chunk of SE3_BASIS_ATT_CHUNK points and 256 consecutive (i, k) pairs, one fp64 accumulator per thread, walks
//               the chunk in ascending point order (coalesced rows of dTq, kSumAhead loads in flight) and writes its partials
//               as [chunk][k][i]; a second kernel adds the chunks in ascending order, one thread per element of dpe.
#include "common.h"
#include "../../include/se3conv_basis_att.h"

// The header's products and sums are single fp32 operations and its fma's are written out: no contraction of `a * b + c * d`
// into an fma, which the 16-byte form would get inside a lane and the one-k-per-lane form (whose products meet through a
// shuffle) would not -- the two forms give the same bits.  The operations are written through mul_rn / add_rn / sub_rn BELOW the
// pragma: HIP's own __fmul_rn / __fadd_rn are plain operators defined above it, which keep their licence to be contracted
// after inlining.
#pragma clang fp contract(off)

namespace se3 {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int kThreads = 256;
constexpr int kIters = 4;             // batches of groups a workgroup walks with one staging of pe
constexpr int kAhead = 4;             // rows of T whose loads a lane issues before it uses the first
constexpr int kSumAhead = 8;          // rows of dTq / chunk partials in flight in the dpe kernels
constexpr int kPeLdsFloats = 8192;    // the largest V * (K | 1) staged in LDS (32 KiB)
static_assert(SE3_BASIS_ATT_CHUNK % 64 == 0 && SE3_BASIS_ATT_CHUNK % kSumAhead == 0, "a chunk is whole wavefronts and whole load batches");
static_assert(SE3_BASIS_ATT_MAX_BASIS <= kWave, "a group of lanes lies inside one wavefront");

struct AttArgs {
  const float* T;
  const float* key;
  const float* pe;
  int64_t key_stride, groups;  // groups = N * H
  int v, h, d, k, lg;          // lg: log2 of the lanes per group
};

template <int VEC>
__device__ __forceinline__ void load_row(const float* p, float (&x)[VEC]) {
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    x[0] = t[0], x[1] = t[1], x[2] = t[2], x[3] = t[3];
  } else {
    x[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_row(float* p, const float (&x)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{x[0], x[1], x[2], x[3]};
  } else {
    *p = x[0];
  }
}
// the levels of tree_k that lie inside a lane, then those across the lanes of its group
template <int VEC>
__device__ __forceinline__ float tree_k(const float (&x)[VEC], int group) {
  float t;
  if constexpr (VEC == 4) t = add_rn(add_rn(x[0], x[1]), add_rn(x[2], x[3]));
  else t = x[0];
  for (int o = 1; o < group; o <<= 1) t = add_rn(t, __shfl_xor(t, o));
  return t;
}
template <bool LDS>
__device__ __forceinline__ float pe_at(const AttArgs& a, const float* pe_s, int k, int i) {
  return LDS ? pe_s[i * (a.k | 1) + k] : a.pe[(size_t)k * a.v + i];
}
template <bool LDS>
__device__ __forceinline__ void stage_pe(const AttArgs& a, float* pe_s) {
  if (!LDS) return;
  const int kp = a.k | 1;
  for (int e = threadIdx.x; e < a.k * a.v; e += kThreads) {
    const int k = e / a.v, i = e - k * a.v;
    pe_s[i * kp + k] = a.pe[e];
  }
  __syncthreads();
}

// what a lane is: its group's (point, head) pair of batch `it`, its first k, and whether it holds anything
struct Lane {
  int64_t n;
  int h, k0, q, group;
  bool live;
};
template <int VEC>
__device__ __forceinline__ Lane lane_of(const AttArgs& a, int it) {
  Lane l;
  l.group = 1 << a.lg;
  l.q = threadIdx.x & (l.group - 1);
  l.k0 = l.q * VEC;
  const int64_t r = ((int64_t)blockIdx.x * kIters + it) * (kThreads >> a.lg) + (threadIdx.x >> a.lg);
  l.live = l.k0 < a.k && r < a.groups;
  l.n = l.live ? r / a.h : 0;
  l.h = l.live ? (int)(r - l.n * a.h) : 0;
  return l;
}

template <int VEC, bool LDS>
__global__ __launch_bounds__(kThreads) void basis_att_fwd_kernel(AttArgs a, float* __restrict__ att, float* __restrict__ out) {
  extern __shared__ float pe_s[];
  stage_pe<LDS>(a, pe_s);
  for (int it = 0; it < kIters; ++it) {
    const Lane l = lane_of<VEC>(a, it);
    const int i0 = l.h * a.d;
    const float* tv = a.T + ((size_t)l.n * 2 * a.v + i0) * a.k + l.k0;
    const float* tq = tv + (size_t)a.v * a.k;
    const float* keyp = a.key + (size_t)l.n * a.key_stride + i0;
    float s[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) s[v] = 0.f;
    for (int d0 = 0; d0 < a.d; d0 += kAhead) {
      float row[kAhead][VEC], kv[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (l.live && d0 + u < a.d) load_row<VEC>(tq + (size_t)(d0 + u) * a.k, row[u]), kv[u] = keyp[d0 + u];
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (l.live && d0 + u < a.d) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) s[v] = fmaf(add_rn(row[u][v], pe_at<LDS>(a, pe_s, l.k0 + v, i0 + d0 + u)), kv[u], s[v]);
        }
    }
    float m = -__builtin_inff();
    if (l.live) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) m = fmaxf(m, s[v]);
    }
    for (int o = 1; o < l.group; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    float w[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) w[v] = l.live ? expf(sub_rn(s[v], m)) : 0.f;
    const float sum = tree_k<VEC>(w, l.group);
    if (l.live) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        w[v] = w[v] / sum;
        att[((size_t)l.n * a.k + l.k0 + v) * a.h + l.h] = w[v];
      }
    }
    for (int d0 = 0; d0 < a.d; d0 += kAhead) {
      float row[kAhead][VEC];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) row[u][v] = 0.f;  // a lane without a k adds +0.0 to the tree
        if (l.live && d0 + u < a.d) load_row<VEC>(tv + (size_t)(d0 + u) * a.k, row[u]);
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (d0 + u < a.d) {  // (uniform: every lane of the wavefront takes part in the shuffles)
          float p[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v) p[v] = mul_rn(row[u][v], w[v]);
          const float t = tree_k<VEC>(p, l.group);
          if (l.live && l.q == 0) out[(size_t)l.n * a.v + i0 + d0 + u] = t;
        }
    }
  }
}

template <int VEC, bool LDS>
__global__ __launch_bounds__(kThreads) void basis_att_bwd_kernel(AttArgs a, const float* __restrict__ grad_out,
                                                                 const float* __restrict__ att, float* __restrict__ dT,
                                                                 float* __restrict__ dkey) {
  extern __shared__ float pe_s[];
  stage_pe<LDS>(a, pe_s);
  for (int it = 0; it < kIters; ++it) {
    const Lane l = lane_of<VEC>(a, it);
    const int i0 = l.h * a.d;
    const size_t at = ((size_t)l.n * 2 * a.v + i0) * a.k + l.k0, half = (size_t)a.v * a.k;
    const float* tv = a.T + at;
    const float* tq = tv + half;
    float* dtv = dT + at;
    float* dtq = dtv + half;
    const float* keyp = a.key + (size_t)l.n * a.key_stride + i0;
    const float* gp = grad_out + (size_t)l.n * a.v + i0;
    float w[VEC], datt[VEC], ds[VEC], p[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) w[v] = l.live ? att[((size_t)l.n * a.k + l.k0 + v) * a.h + l.h] : 0.f, datt[v] = 0.f;
    if (l.live) {
      for (int d0 = 0; d0 < a.d; d0 += kAhead) {
        float row[kAhead][VEC], gv[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
          if (d0 + u < a.d) load_row<VEC>(tv + (size_t)(d0 + u) * a.k, row[u]), gv[u] = gp[d0 + u];
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
          if (d0 + u < a.d) {
            float o[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) datt[v] = fmaf(gv[u], row[u][v], datt[v]), o[v] = mul_rn(gv[u], w[v]);
            store_row<VEC>(dtv + (size_t)(d0 + u) * a.k, o);
          }
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) p[v] = mul_rn(w[v], datt[v]);
    const float qd = tree_k<VEC>(p, l.group);
#pragma unroll
    for (int v = 0; v < VEC; ++v) ds[v] = l.live ? mul_rn(w[v], sub_rn(datt[v], qd)) : 0.f;
    for (int d0 = 0; d0 < a.d; d0 += kAhead) {
      float row[kAhead][VEC], kv[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) row[u][v] = 0.f;
        kv[u] = 0.f;
        if (l.live && d0 + u < a.d) load_row<VEC>(tq + (size_t)(d0 + u) * a.k, row[u]), kv[u] = keyp[d0 + u];
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (d0 + u < a.d) {
          float o[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            o[v] = mul_rn(ds[v], kv[u]);
            const float pe = l.live ? pe_at<LDS>(a, pe_s, l.k0 + v, i0 + d0 + u) : 0.f;
            p[v] = mul_rn(ds[v], add_rn(row[u][v], pe));
          }
          if (l.live) store_row<VEC>(dtq + (size_t)(d0 + u) * a.k, o);
          const float t = tree_k<VEC>(p, l.group);
          if (l.live && l.q == 0) dkey[(size_t)l.n * a.v + i0 + d0 + u] = t;
        }
    }
  }
}

// partials [chunk][K][V]; block = (chunk, slab of kThreads (i, k) pairs in the order of a dTq row)
__global__ __launch_bounds__(kThreads) void basis_att_dpe_chunks_kernel(const float* __restrict__ dT, int n, int v, int k, int slabs,
                                                                        double* __restrict__ partials) {
  const int c = blockIdx.x / slabs, slab = blockIdx.x - c * slabs;
  const int pair = slab * kThreads + threadIdx.x, pairs = v * k;
  if (pair >= pairs) return;
  const int n0 = c * SE3_BASIS_ATT_CHUNK, n1 = min(n0 + SE3_BASIS_ATT_CHUNK, n);
  const float* src = dT + (size_t)v * k + pair;  // the query half of point 0
  const size_t stride = (size_t)2 * v * k;
  double s = 0.0;
  for (int p0 = n0; p0 < n1; p0 += kSumAhead) {  // the additions are a serial chain in ascending point order; the loads are not
    float x[kSumAhead];
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u) x[u] = p0 + u < n1 ? src[(size_t)(p0 + u) * stride] : 0.f;
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u)
      if (p0 + u < n1) s += (double)x[u];
  }
  const int i = pair / k, kk = pair - i * k;
  partials[(size_t)c * pairs + (size_t)kk * v + i] = s;
}

__global__ __launch_bounds__(kThreads) void basis_att_dpe_finish_kernel(const double* __restrict__ partials, int chunks, int total,
                                                                        float* __restrict__ dpe) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  double s = 0.0;
  for (int c0 = 0; c0 < chunks; c0 += kSumAhead) {
    double part[kSumAhead];
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u) part[u] = c0 + u < chunks ? partials[(size_t)(c0 + u) * total + i] : 0.0;
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u)
      if (c0 + u < chunks) s += part[u];
  }
  dpe[i] = (float)s;
}

constexpr int64_t kLim = 1ll << 31;
inline bool beyond(int64_t a, int64_t b) { return a > 0 && b > 0 && a >= (kLim + b - 1) / b; }  // a * b >= 2^31, no overflow

// key_stride < 0: not looked at (the workspace query has none)
int att_shape(int64_t n, int32_t v, int32_t h, int32_t k, int64_t key_stride) {
  if (n < 0 || v < 1 || h < 1 || v % h != 0 || k < 1 || (key_stride >= 0 && key_stride < v)) return SE3_ERR_INVALID_ARGUMENT;
  if (k > SE3_BASIS_ATT_MAX_BASIS || beyond(n, (int64_t)2 * v * k) || beyond(n, (int64_t)k * h) || beyond(k, v) ||
      (key_stride > 0 && beyond(n, key_stride)))
    return SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}

int64_t chunks_of(int64_t n) { return (n + SE3_BASIS_ATT_CHUNK - 1) / SE3_BASIS_ATT_CHUNK; }

size_t att_workspace(int64_t n, int32_t v, int32_t k) {
  return (size_t)(n > 0 ? chunks_of(n) : 1) * (size_t)k * (size_t)v * sizeof(double);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Form {
  bool vec, lds;
  int lg;
  unsigned blocks;
  size_t lds_bytes;
};
Form form_of(int64_t n, int32_t v, int32_t h, int32_t k, bool aligned) {
  Form f;
  f.vec = k % 4 == 0 && aligned;
  const int lanes = f.vec ? k / 4 : k;
  f.lg = 0;
  while ((1 << f.lg) < lanes) ++f.lg;
  f.lds = (int64_t)v * (k | 1) <= kPeLdsFloats;
  f.lds_bytes = f.lds ? (size_t)v * (k | 1) * sizeof(float) : 0;
  const int64_t per_block = (int64_t)(kThreads >> f.lg) * kIters;
  f.blocks = (unsigned)((n * h + per_block - 1) / per_block);
  return f;
}

}  // namespace
}  // namespace se3

using namespace se3;

// one launch of `kernel<VEC, LDS>` for the form `f`
#define SE3_ATT_LAUNCH(kernel, f, stream, ...)                                                                              \
  do {                                                                                                                      \
    if (f.vec && f.lds) hipLaunchKernelGGL((kernel<4, true>), dim3(f.blocks), dim3(kThreads), f.lds_bytes, stream, __VA_ARGS__);   \
    else if (f.vec) hipLaunchKernelGGL((kernel<4, false>), dim3(f.blocks), dim3(kThreads), 0, stream, __VA_ARGS__);         \
    else if (f.lds) hipLaunchKernelGGL((kernel<1, true>), dim3(f.blocks), dim3(kThreads), f.lds_bytes, stream, __VA_ARGS__);       \
    else hipLaunchKernelGGL((kernel<1, false>), dim3(f.blocks), dim3(kThreads), 0, stream, __VA_ARGS__);                    \
  } while (0)

extern "C" size_t se3_basis_att_workspace_bytes(int64_t n_rows, int32_t value_size, int32_t num_heads, int32_t num_basis) {
  if (att_shape(n_rows, value_size, num_heads, num_basis, -1) != SE3_OK) return 0;
  return att_workspace(n_rows, value_size, num_basis);
}

extern "C" int se3_basis_att_fwd(const float* T, const float* key, int64_t key_stride, const float* pe, int64_t n_rows,
                                 int32_t value_size, int32_t num_heads, int32_t num_basis, float* att, float* out, void* stream_) {
  if (key_stride < 0) return SE3_ERR_INVALID_ARGUMENT;
  if (int rc = att_shape(n_rows, value_size, num_heads, num_basis, key_stride)) return rc;
  if (!pe || (n_rows > 0 && (!T || !key || !att || !out))) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return SE3_OK;
  const Form f = form_of(n_rows, value_size, num_heads, num_basis, aligned16(T));
  const AttArgs a{T, key, pe, key_stride, n_rows * num_heads, value_size, num_heads, value_size / num_heads, num_basis, f.lg};
  hipStream_t stream = (hipStream_t)stream_;
  SE3_ATT_LAUNCH(basis_att_fwd_kernel, f, stream, a, att, out);
  return check_launch();
}

extern "C" int se3_basis_att_bwd(const float* grad_out, const float* T, const float* key, int64_t key_stride, const float* pe,
                                 const float* att, int64_t n_rows, int32_t value_size, int32_t num_heads, int32_t num_basis,
                                 float* dT, float* dkey, float* dpe, void* workspace, size_t workspace_bytes, void* stream_) {
  if (key_stride < 0) return SE3_ERR_INVALID_ARGUMENT;
  if (int rc = att_shape(n_rows, value_size, num_heads, num_basis, key_stride)) return rc;
  if (!pe || !dpe || !workspace || (n_rows > 0 && (!grad_out || !T || !key || !att || !dT || !dkey))) return SE3_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < att_workspace(n_rows, value_size, num_basis)) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  double* partials = (double*)workspace;
  const int chunks = (int)chunks_of(n_rows), pairs = value_size * num_basis;
  if (n_rows > 0) {
    const Form f = form_of(n_rows, value_size, num_heads, num_basis, aligned16(T) && aligned16(dT));
    const AttArgs a{T, key, pe, key_stride, n_rows * num_heads, value_size, num_heads, value_size / num_heads, num_basis, f.lg};
    SE3_ATT_LAUNCH(basis_att_bwd_kernel, f, stream, a, grad_out, att, dT, dkey);
    const int slabs = (pairs + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(basis_att_dpe_chunks_kernel, dim3((unsigned)((int64_t)chunks * slabs)), dim3(kThreads), 0, stream, dT,
                       (int)n_rows, value_size, num_basis, slabs, partials);
  }
  hipLaunchKernelGGL(basis_att_dpe_finish_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                     partials, chunks, pairs, dpe);
  return check_launch();
}
