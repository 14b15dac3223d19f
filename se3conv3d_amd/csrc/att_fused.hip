// The attention of MultiHeadAttLayer / LoRAttConvLayer as one edge-wise operator, without the aggregate T
// (include/se3conv_att_fused.h).
//
//   fwd, bwd_samples   ONE WAVEFRONT PER SAMPLE, the heads one after the other.  Two lane mappings alternate inside a head:
//                      lane = edge of the current slab of SE3_ATT_FUSED_SLAB edges (the per-edge dot products over the D
//                      channels of the head -- c, da -- which read D contiguous floats of a neighbour's row, 16 bytes at a time
//                      where D % 4 == 0 and the bases are aligned), and lane = k (everything that is a vector over the basis
//                      functions: s, att, datt, ds, and the rows of phi / dphi, K contiguous floats per edge).  A per-edge scalar
//                      goes from the first mapping to the second by v_readlane (the edge loop is wave-uniform), a tree over k
//                      goes back by one lane keeping the result.  The sums over a sample's edges are fma chains in ascending
//                      edge order that run on across the slabs, so a hub row of any degree costs no buffer: nothing is sized
//                      by the degree.  The sums over k are the pairwise tree of se3conv_basis_att.h by xor shuffles.  The
//                      output rows (out, dkey) take lane = channel of the head, 64 channels at a time.
//                      `pe` is staged in LDS once per workgroup as pe_s[i][k] with an odd row length, for the kIters samples
//                      each of its wavefronts walks (a `pe` beyond kPeLdsFloats is read from memory: same values, slower).
//                      The backward pass parks c and da of an edge in the workspace slots of dc and a between its two walks of
//                      a slab -- written and read back by the same lane -- and accumulates dphi over the heads in place, a row
//                      element always by the same lane.
//   bwd_sources        a group of lanes per source, lane = channel: two fma chains over the source's entries of the transposed
//                      list, in list order, gathering g / key rows (coalesced) weighted by a / dc through t_edge_ids.  No atomics.
//   dpe                as basis_att.hip: fp64 partials per chunk of SE3_ATT_FUSED_CHUNK points in ascending point order, one thread
//                      per (k, i), then the chunks in ascending order.  The addends ds[k,h(i)] * key[i] are formed on the fly.
#include "common.h"
#include "../../include/se3conv_att_fused.h"
#include "../../include/se3conv_basis_att.h"

// The header's products and sums are single fp32 operations and its fma's are written out: nothing is contracted (see
// basis_att.hip on why the operations go through functions defined BELOW the pragma).
#pragma clang fp contract(off)

namespace se3 {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kIters = 8;             // samples a wavefront walks with one staging of pe
constexpr int kSlab = SE3_ATT_FUSED_SLAB;
constexpr int kAhead = 4;             // edges of a slab / entries of a source whose loads are issued before the first is used
constexpr int kSumAhead = 8;          // points / chunk partials in flight in the dpe kernels
constexpr int kPeLdsFloats = 8192;    // the largest V * (K | 1) staged in LDS (32 KiB)
static_assert(kSlab == kWave, "a slab is one edge per lane");
static_assert(SE3_ATT_FUSED_CHUNK % 64 == 0 && SE3_ATT_FUSED_CHUNK % kSumAhead == 0, "a chunk is whole wavefronts and whole load batches");
static_assert(SE3_BASIS_ATT_MAX_BASIS <= kWave, "the basis functions lie along the lanes of one wavefront");

struct FusedArgs {
  const float* phi;
  const float* x;
  const float* pe;
  const int32_t* nbr;
  const int32_t* ends;
  int64_t n;
  int v, h, d, k, group;  // group: the smallest power of two >= k
  int lds;                // pe is staged
};

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// the value lane `j` holds, for a wave-uniform j
__device__ __forceinline__ float from_lane(float x, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j)); }
__device__ __forceinline__ int from_lane(int x, int j) { return __builtin_amdgcn_readlane(x, j); }

// tree_k over the lanes [0, group) (lanes >= K hold +0.0f), handed to every lane
__device__ __forceinline__ float tree_k(float t, int group) {
  for (int o = 1; o < group; o <<= 1) t = add_rn(t, __shfl_xor(t, o));
  return from_lane(t, 0);
}

__device__ __forceinline__ float pe_at(const FusedArgs& a, const float* pe_s, int k, int i) {
  return a.lds ? pe_s[i * (a.k | 1) + k] : a.pe[(size_t)k * a.v + i];
}
__device__ __forceinline__ void stage_pe(const FusedArgs& a, float* pe_s) {
  if (!a.lds) return;
  const int kp = a.k | 1;
  for (int e = threadIdx.x; e < a.k * a.v; e += kThreads) {
    const int k = e / a.v, i = e - k * a.v;
    pe_s[i * kp + k] = a.pe[e];
  }
  __syncthreads();
}

// fma(p[i], q[i], .) over i = 0 .. d - 1, ascending, from +0.0f
template <bool VEC>
__device__ __forceinline__ float dot_chain(const float* __restrict__ p, const float* __restrict__ q, int d) {
  float c = 0.f;
  if constexpr (VEC) {
    for (int i = 0; i < d; i += 4) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(p + i), w = *reinterpret_cast<const f32x4*>(q + i);
      c = fmaf(u[0], w[0], c), c = fmaf(u[1], w[1], c), c = fmaf(u[2], w[2], c), c = fmaf(u[3], w[3], c);
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < d; ++i) c = fmaf(p[i], q[i], c);
  }
  return c;
}

// the sample of wavefront `wave` in batch `it` of a workgroup, and its edges
struct Sample {
  int64_t s;
  int e_begin, e_end;
};
__device__ __forceinline__ bool sample_of(const FusedArgs& a, int it, int wave, Sample& o) {
  o.s = ((int64_t)blockIdx.x * kIters + it) * kWaves + wave;
  if (o.s >= a.n) return false;
  o.e_begin = uniform(o.s > 0 ? a.ends[o.s - 1] : 0);
  o.e_end = uniform(a.ends[o.s]);
  return true;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void att_fused_fwd_kernel(FusedArgs a, float* __restrict__ att, float* __restrict__ out) {
  extern __shared__ float pe_s[];
  stage_pe(a, pe_s);
  const int lane = threadIdx.x & (kWave - 1), wave = uniform(threadIdx.x / kWave);
  const size_t v3 = (size_t)3 * a.v;
  const bool kl = lane < a.k;
  for (int it = 0; it < kIters; ++it) {
    Sample sm;
    if (!sample_of(a, it, wave, sm)) break;
    const float* key = a.x + (size_t)sm.s * v3 + 2 * a.v;
    for (int h = 0; h < a.h; ++h) {
      const int i0 = h * a.d;
      float sc = 0.f;
      for (int e0 = sm.e_begin; e0 < sm.e_end; e0 += kSlab) {
        const int cnt = min(kSlab, sm.e_end - e0);
        float c = 0.f;
        if (lane < cnt) {
          const int p = a.nbr[2 * (size_t)(e0 + lane) + 1];
          c = dot_chain<VEC>(a.x + (size_t)p * v3 + a.v + i0, key + i0, a.d);
        }
        const float* ph = a.phi + (size_t)e0 * a.k + (kl ? lane : 0);
        for (int j0 = 0; j0 < cnt; j0 += kAhead) {  // (the trip counts are wave-uniform: from_lane takes a scalar lane)
          float r[kAhead];
#pragma unroll
          for (int u = 0; u < kAhead; ++u) r[u] = j0 + u < cnt ? ph[(size_t)(j0 + u) * a.k] : 0.f;
#pragma unroll
          for (int u = 0; u < kAhead; ++u)
            if (j0 + u < cnt) sc = fmaf(r[u], from_lane(c, j0 + u), sc);
        }
      }
      float t = 0.f;
      if (kl)
        for (int i = 0; i < a.d; ++i) t = fmaf(pe_at(a, pe_s, lane, i0 + i), key[i0 + i], t);
      sc = add_rn(sc, t);
      float m = kl ? sc : -__builtin_inff();
      for (int o = 1; o < kWave; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
      float w = kl ? expf(sub_rn(sc, m)) : 0.f;
      const float sum = tree_k(w, a.group);
      w = kl ? w / sum : 0.f;
      if (kl) att[((size_t)sm.s * a.k + lane) * a.h + h] = w;
      for (int cb = 0; cb < a.d; cb += kWave) {
        const int ci = cb + lane;
        const bool cl = ci < a.d;
        float acc = 0.f;
        for (int e0 = sm.e_begin; e0 < sm.e_end; e0 += kSlab) {
          const int cnt = min(kSlab, sm.e_end - e0);
          const int p = lane < cnt ? a.nbr[2 * (size_t)(e0 + lane) + 1] : 0;
          const float* ph = a.phi + (size_t)e0 * a.k + (kl ? lane : 0);
          float am = 0.f;
          for (int j0 = 0; j0 < cnt; j0 += kAhead) {
            float r[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) r[u] = j0 + u < cnt ? ph[(size_t)(j0 + u) * a.k] : 0.f;
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
              if (j0 + u < cnt) {
                const float tj = tree_k(kl ? mul_rn(r[u], w) : 0.f, a.group);
                if (lane == j0 + u) am = tj;
              }
          }
          const float* xv = a.x + i0 + (cl ? ci : 0);
          for (int j0 = 0; j0 < cnt; j0 += kAhead) {
            float r[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) r[u] = j0 + u < cnt ? xv[(size_t)from_lane(p, j0 + u) * v3] : 0.f;
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
              if (j0 + u < cnt) acc = fmaf(from_lane(am, j0 + u), r[u], acc);
          }
        }
        if (cl) out[(size_t)sm.s * a.v + i0 + ci] = acc;
      }
    }
  }
}

// wa / wdc: the workspace's a [E,H] and dc [E,H]; between the two walks of a slab they hold da and c.  wds [N,K,H].
template <bool VEC>
__global__ __launch_bounds__(kThreads) void att_fused_bwd_samples_kernel(FusedArgs a, const float* __restrict__ grad_out,
                                                                         const float* __restrict__ att, float* wa, float* wdc,
                                                                         float* __restrict__ wds, float* dphi,
                                                                         float* __restrict__ dx) {
  extern __shared__ float pe_s[];
  stage_pe(a, pe_s);
  const int lane = threadIdx.x & (kWave - 1), wave = uniform(threadIdx.x / kWave);
  const size_t v3 = (size_t)3 * a.v;
  const bool kl = lane < a.k;
  for (int it = 0; it < kIters; ++it) {
    Sample sm;
    if (!sample_of(a, it, wave, sm)) break;
    const float* key = a.x + (size_t)sm.s * v3 + 2 * a.v;
    const float* g = grad_out + (size_t)sm.s * a.v;
    for (int h = 0; h < a.h; ++h) {
      const int i0 = h * a.d;
      const float w = kl ? att[((size_t)sm.s * a.k + lane) * a.h + h] : 0.f;
      float datt = 0.f;
      for (int e0 = sm.e_begin; e0 < sm.e_end; e0 += kSlab) {
        const int cnt = min(kSlab, sm.e_end - e0);
        float da = 0.f;
        if (lane < cnt) {
          const int p = a.nbr[2 * (size_t)(e0 + lane) + 1];
          const float* row = a.x + (size_t)p * v3 + i0;
          const float c = dot_chain<VEC>(row + a.v, key + i0, a.d);
          da = dot_chain<VEC>(g + i0, row, a.d);
          wdc[(size_t)(e0 + lane) * a.h + h] = c;
          wa[(size_t)(e0 + lane) * a.h + h] = da;
        }
        const float* ph = a.phi + (size_t)e0 * a.k + (kl ? lane : 0);
        for (int j0 = 0; j0 < cnt; j0 += kAhead) {
          float r[kAhead];
#pragma unroll
          for (int u = 0; u < kAhead; ++u) r[u] = j0 + u < cnt ? ph[(size_t)(j0 + u) * a.k] : 0.f;
#pragma unroll
          for (int u = 0; u < kAhead; ++u)
            if (j0 + u < cnt) datt = fmaf(r[u], from_lane(da, j0 + u), datt);
        }
      }
      const float q = tree_k(kl ? mul_rn(w, datt) : 0.f, a.group);
      const float ds = kl ? mul_rn(w, sub_rn(datt, q)) : 0.f;
      if (kl) wds[((size_t)sm.s * a.k + lane) * a.h + h] = ds;
      for (int e0 = sm.e_begin; e0 < sm.e_end; e0 += kSlab) {
        const int cnt = min(kSlab, sm.e_end - e0);
        float c = 0.f, da = 0.f, am = 0.f, dcm = 0.f;
        if (lane < cnt) c = wdc[(size_t)(e0 + lane) * a.h + h], da = wa[(size_t)(e0 + lane) * a.h + h];
        const size_t at = (size_t)e0 * a.k + (kl ? lane : 0);
        for (int j = 0; j < cnt; ++j) {
          const float r = a.phi[at + (size_t)j * a.k];
          const float ta = tree_k(kl ? mul_rn(r, w) : 0.f, a.group), tc = tree_k(kl ? mul_rn(r, ds) : 0.f, a.group);
          if (lane == j) am = ta, dcm = tc;
          const float daj = from_lane(da, j), cj = from_lane(c, j);
          if (kl) {
            float dp = h ? dphi[at + (size_t)j * a.k] : 0.f;
            dp = fmaf(w, daj, dp);
            dp = fmaf(ds, cj, dp);
            dphi[at + (size_t)j * a.k] = dp;
          }
        }
        if (lane < cnt) wa[(size_t)(e0 + lane) * a.h + h] = am, wdc[(size_t)(e0 + lane) * a.h + h] = dcm;
      }
      for (int cb = 0; cb < a.d; cb += kWave) {
        const int ci = cb + lane;
        const bool cl = ci < a.d;
        float acc = 0.f;
        for (int e0 = sm.e_begin; e0 < sm.e_end; e0 += kSlab) {
          const int cnt = min(kSlab, sm.e_end - e0);
          int p = 0;
          float dcm = 0.f;
          if (lane < cnt) p = a.nbr[2 * (size_t)(e0 + lane) + 1], dcm = wdc[(size_t)(e0 + lane) * a.h + h];  // this lane's own store
          const float* xq = a.x + a.v + i0 + (cl ? ci : 0);
          for (int j0 = 0; j0 < cnt; j0 += kAhead) {
            float r[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) r[u] = j0 + u < cnt ? xq[(size_t)from_lane(p, j0 + u) * v3] : 0.f;
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
              if (j0 + u < cnt) acc = fmaf(from_lane(dcm, j0 + u), r[u], acc);
          }
        }
        float u = 0.f;
        const int nch = min(kWave, a.d - cb);
        for (int ii = 0; ii < nch; ++ii) {
          const float tu = tree_k(kl ? mul_rn(ds, pe_at(a, pe_s, lane, i0 + cb + ii)) : 0.f, a.group);
          if (lane == ii) u = tu;
        }
        if (cl) dx[(size_t)sm.s * v3 + 2 * a.v + i0 + ci] = add_rn(acc, u);
      }
    }
  }
}

// a group of 2^lg lanes per source, lane = channel (a wider row in steps of the group)
__global__ __launch_bounds__(kThreads) void att_fused_bwd_sources_kernel(const float* __restrict__ grad_out, const float* __restrict__ x,
                                                                         const float* __restrict__ wa, const float* __restrict__ wdc,
                                                                         const int32_t* __restrict__ t_samples,
                                                                         const int32_t* __restrict__ t_ends,
                                                                         const int32_t* __restrict__ t_edge_ids, int64_t n, int v,
                                                                         int h, int d, int lg, float* __restrict__ dx) {
  const int64_t p = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> lg;
  if (p >= n) return;
  const int q = threadIdx.x & ((1 << lg) - 1);
  const size_t v3 = (size_t)3 * v;
  const int j_begin = p > 0 ? t_ends[p - 1] : 0, j_end = t_ends[p];
  for (int ci = q; ci < v; ci += 1 << lg) {
    const int hh = ci / d;
    float av = 0.f, aq = 0.f;
    for (int j0 = j_begin; j0 < j_end; j0 += kAhead) {
      float wv[kAhead], wq[kAhead], gv[kAhead], kv[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (j0 + u < j_end) {
          const size_t s = (size_t)t_samples[j0 + u], e = (size_t)t_edge_ids[j0 + u];
          wv[u] = wa[e * h + hh], wq[u] = wdc[e * h + hh];
          gv[u] = grad_out[s * v + ci], kv[u] = x[s * v3 + 2 * v + ci];
        }
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (j0 + u < j_end) av = fmaf(wv[u], gv[u], av), aq = fmaf(wq[u], kv[u], aq);
    }
    dx[(size_t)p * v3 + ci] = av;
    dx[(size_t)p * v3 + v + ci] = aq;
  }
}

// partials [chunk][K][V]; block = (chunk, slab of kThreads (k, i) pairs in the order of dpe)
__global__ __launch_bounds__(kThreads) void att_fused_dpe_chunks_kernel(const float* __restrict__ wds, const float* __restrict__ x, int n,
                                                                        int v, int h, int d, int k, int slabs,
                                                                        double* __restrict__ partials) {
  const int c = blockIdx.x / slabs, slab = blockIdx.x - c * slabs;
  const int pair = slab * kThreads + threadIdx.x, pairs = v * k;
  if (pair >= pairs) return;
  const int kk = pair / v, i = pair - kk * v;
  const int n0 = c * SE3_ATT_FUSED_CHUNK, n1 = min(n0 + SE3_ATT_FUSED_CHUNK, n);
  const float* dsp = wds + (size_t)kk * h + i / d;
  const float* keyp = x + 2 * v + i;
  const size_t ds_stride = (size_t)k * h, key_stride = (size_t)3 * v;
  double s = 0.0;
  for (int p0 = n0; p0 < n1; p0 += kSumAhead) {  // the additions are a serial chain in ascending point order; the loads are not
    float t[kSumAhead];
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u) t[u] = p0 + u < n1 ? mul_rn(dsp[(size_t)(p0 + u) * ds_stride], keyp[(size_t)(p0 + u) * key_stride]) : 0.f;
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u)
      if (p0 + u < n1) s += (double)t[u];
  }
  partials[(size_t)c * pairs + pair] = s;
}

__global__ __launch_bounds__(kThreads) void att_fused_dpe_finish_kernel(const double* __restrict__ partials, int chunks, int total,
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

int fused_shape(int64_t n, int64_t e, int32_t v, int32_t h, int32_t k) {
  if (n < 0 || e < 0 || (e > 0 && n == 0) || v < 1 || h < 1 || v % h != 0 || k < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (k > SE3_BASIS_ATT_MAX_BASIS || beyond(n, (int64_t)3 * v) || beyond(n, (int64_t)k * h) || beyond(e, k) || beyond(e, h) ||
      beyond(e, 2) || beyond(k, v))
    return SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}

int64_t chunks_of(int64_t n) { return (n + SE3_ATT_FUSED_CHUNK - 1) / SE3_ATT_FUSED_CHUNK; }

// the workspace of the backward call: a [E,H] | dc [E,H] | ds [N,K,H] | partials [chunks][K][V] (fp64)
struct Layout {
  size_t a, dc, ds, partials, bytes;
};
Layout layout_of(int64_t n, int64_t e, int32_t v, int32_t h, int32_t k) {
  Layout l;
  const size_t eh = align_up((size_t)e * h * sizeof(float), 16), nkh = align_up((size_t)n * k * h * sizeof(float), 16);
  l.a = 0, l.dc = eh, l.ds = 2 * eh, l.partials = 2 * eh + nkh;
  l.bytes = l.partials + (size_t)(n > 0 ? chunks_of(n) : 1) * (size_t)k * (size_t)v * sizeof(double);
  return l;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

FusedArgs args_of(const float* phi, const float* x, const float* pe, const int32_t* nbr, const int32_t* ends, int64_t n, int32_t v,
                  int32_t h, int32_t k) {
  FusedArgs a{phi, x, pe, nbr, ends, n, v, h, v / h, k, 1, 0};
  while (a.group < k) a.group <<= 1;
  a.lds = (int64_t)v * (k | 1) <= kPeLdsFloats;
  return a;
}
size_t lds_bytes(const FusedArgs& a) { return a.lds ? (size_t)a.v * (a.k | 1) * sizeof(float) : 0; }
unsigned sample_blocks(int64_t n) { return (unsigned)((n + (int64_t)kWaves * kIters - 1) / ((int64_t)kWaves * kIters)); }

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" size_t se3_att_fused_workspace_bytes(int64_t n_rows, int64_t n_edges, int32_t value_size, int32_t num_heads,
                                                int32_t num_basis) {
  if (fused_shape(n_rows, n_edges, value_size, num_heads, num_basis) != SE3_OK) return 0;
  return layout_of(n_rows, n_edges, value_size, num_heads, num_basis).bytes;
}

extern "C" int se3_att_fused_fwd(const float* phi, const float* x, const float* pe, const int32_t* neighbors, const int32_t* ends,
                                 int64_t n_rows, int64_t n_edges, int32_t value_size, int32_t num_heads, int32_t num_basis,
                                 float* att, float* out, void* stream_) {
  if (int rc = fused_shape(n_rows, n_edges, value_size, num_heads, num_basis)) return rc;
  if (!pe || (n_rows > 0 && (!x || !ends || !att || !out)) || (n_edges > 0 && (!phi || !neighbors))) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return SE3_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const FusedArgs a = args_of(phi, x, pe, neighbors, ends, n_rows, value_size, num_heads, num_basis);
  ProfScope prof("att_fused_fwd", stream);
  if (a.d % 4 == 0 && aligned16(x))
    hipLaunchKernelGGL((att_fused_fwd_kernel<true>), dim3(sample_blocks(n_rows)), dim3(kThreads), lds_bytes(a), stream, a, att, out);
  else
    hipLaunchKernelGGL((att_fused_fwd_kernel<false>), dim3(sample_blocks(n_rows)), dim3(kThreads), lds_bytes(a), stream, a, att, out);
  return check_launch();
}

extern "C" int se3_att_fused_bwd(const float* grad_out, const float* phi, const float* x, const float* pe, const float* att,
                                 const int32_t* neighbors, const int32_t* ends, const int32_t* t_samples, const int32_t* t_ends,
                                 const int32_t* t_edge_ids, int64_t n_rows, int64_t n_edges, int32_t value_size, int32_t num_heads,
                                 int32_t num_basis, float* dphi, float* dx, float* dpe, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
  if (int rc = fused_shape(n_rows, n_edges, value_size, num_heads, num_basis)) return rc;
  if (!pe || !dpe || !workspace || (n_rows > 0 && (!grad_out || !x || !att || !ends || !t_ends || !dx)) ||
      (n_edges > 0 && (!phi || !neighbors || !t_samples || !t_edge_ids || !dphi)))
    return SE3_ERR_INVALID_ARGUMENT;
  const Layout l = layout_of(n_rows, n_edges, value_size, num_heads, num_basis);
  if (workspace_bytes < l.bytes) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  float* wa = (float*)(ws + l.a);
  float* wdc = (float*)(ws + l.dc);
  float* wds = (float*)(ws + l.ds);
  double* partials = (double*)(ws + l.partials);
  const int chunks = (int)chunks_of(n_rows), pairs = value_size * num_basis;
  if (n_rows > 0) {
    const FusedArgs a = args_of(phi, x, pe, neighbors, ends, n_rows, value_size, num_heads, num_basis);
    {
      ProfScope prof("att_fused_bwd_samples", stream);
      if (a.d % 4 == 0 && aligned16(x) && aligned16(grad_out))
        hipLaunchKernelGGL((att_fused_bwd_samples_kernel<true>), dim3(sample_blocks(n_rows)), dim3(kThreads), lds_bytes(a), stream, a,
                           grad_out, att, wa, wdc, wds, dphi, dx);
      else
        hipLaunchKernelGGL((att_fused_bwd_samples_kernel<false>), dim3(sample_blocks(n_rows)), dim3(kThreads), lds_bytes(a), stream, a,
                           grad_out, att, wa, wdc, wds, dphi, dx);
    }
    {
      ProfScope prof("att_fused_bwd_sources", stream);
      int lg = 0;
      while ((1 << lg) < value_size && lg < 6) ++lg;
      const int64_t threads = n_rows << lg;
      hipLaunchKernelGGL(att_fused_bwd_sources_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                         grad_out, x, wa, wdc, t_samples, t_ends, t_edge_ids, n_rows, value_size, num_heads, a.d, lg, dx);
    }
    const int slabs = (pairs + kThreads - 1) / kThreads;
    ProfScope prof("att_fused_dpe", stream);
    hipLaunchKernelGGL(att_fused_dpe_chunks_kernel, dim3((unsigned)((int64_t)chunks * slabs)), dim3(kThreads), 0, stream, wds, x,
                       (int)n_rows, value_size, num_heads, a.d, num_basis, slabs, partials);
  }
  ProfScope prof("att_fused_dpe_sum", stream);
  hipLaunchKernelGGL(att_fused_dpe_finish_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                     partials, chunks, pairs, dpe);
  return check_launch();
}
