// Point-neighbourhood embeddings and the max aggregation (include/se3conv_pne.h).
//
//   embed fwd   a workgroup of 256 threads takes a tile of 64 edges.  Phase 1 writes the inputs of the projection into LDS
//               as `in[j][edge]` -- the relative position (MLP kinds) or the correlation with every kernel point, one value
//               per thread and step; for `box` one thread per edge then turns its column of squared distances into the one-hot
//               row.  For softmax one thread per edge walks the row once for the maximum and once for the sum.  Phase 2
//               runs one thread per (edge, k), k fastest, so `phi` is written in whole rows: the dot product over j reads
//               the LDS column (a broadcast within the lanes of one edge) and `A` through the vector cache.
//   embed bwd   a workgroup takes a chunk of SE3_PNE_CHUNK edges, tile after tile, 32 basis functions at a time: phase 1 as
//               above, then `gz` of the tile into LDS, then every thread adds its (j, k) pairs -- fp64 accumulators that live
//               in registers across the tiles of the chunk, so the order is the ascending edge order of the header.  A second
//               kernel adds the chunk partials in ascending order, one thread per (j, k).
//   max fwd     one wavefront per sample, lanes across `o`: the sample index is made scalar, so `ends`, the edge row and
//               `phi[e, k]` are scalar loads and `G[src, k, o]` is one coalesced row per k, sixteen rows in flight.
//   max bwd     dphi: one wavefront per sample, lanes across `k`; it clears the rows of its edges and then walks `o` in
//               ascending order, eight at a time, adding into the row of the winner -- every address is read and written by
//               one lane only.
//               dG: one wavefront per (source, tile of 64 `o`), 32 basis functions in registers at a time, the incoming edges
//               in the order of the transposition; an edge that wins in no lane is skipped by a ballot.
#include "common.h"
#include "../../include/se3conv_pne.h"

namespace se3 {
namespace {

constexpr int kTile = 64;       // edges per tile of the embedding kernels
constexpr int kThreads = 256;
constexpr int kSlab = 32;       // basis functions per pass of embed bwd and of the dG kernel
constexpr int kGroup = 8;       // channels per step of the dphi kernel
constexpr int kAhead = 16;      // rows of G whose loads the max kernel issues before it uses the first
constexpr int kMaxIn = SE3_PNE_MAX_KPTS;
constexpr int kPairs = ((kMaxIn + 1) * kSlab + kThreads - 1) / kThreads;  // (j, k) pairs per thread of embed bwd, bias row included
static_assert(SE3_PNE_CHUNK % kTile == 0, "a chunk is whole tiles");
static_assert(kMaxIn >= 3, "the MLP kinds have three inputs");

__host__ __device__ inline bool is_kp(int kind) { return kind >= SE3_PNE_KP_GAUSS; }
inline int inputs_of(int kind, int n_kpts) { return is_kp(kind) ? n_kpts : 3; }

struct EmbedArgs {
  const float* pts;
  const float* samples;
  const int32_t* neighbors;
  const float* rho;
  const float* kpts;
  const float* A;
  const float* beta;
  int e_total, kind, n_in, k;
  float sigma;
};

// Phase 1: `in[j][kTile]` of the tile that starts at edge `e0` (absent edges of the last tile: zeros).  Ends with a barrier.
__device__ __forceinline__ void tile_inputs(const EmbedArgs& a, int e0, float (*in)[kTile]) {
  const int t = threadIdx.x;
  const int le = t & (kTile - 1), part = t / kTile;  // four threads per edge
  const int e = e0 + le;
  const bool live = e < a.e_total;
  float r[3] = {0.f, 0.f, 0.f};
  if (live) {
    const int smp = a.neighbors[2 * e], src = a.neighbors[2 * e + 1];
    const float rho = *a.rho;
#pragma unroll
    for (int d = 0; d < 3; ++d) r[d] = (a.pts[3 * src + d] - a.samples[3 * smp + d]) * rho;
  }
  if (!is_kp(a.kind)) {
    if (part < 3) in[part][le] = r[part];
  } else {
    for (int j = part; j < a.n_in; j += kThreads / kTile) {
      const float u0 = r[0] - a.kpts[3 * j], u1 = r[1] - a.kpts[3 * j + 1], u2 = r[2] - a.kpts[3 * j + 2];
      const float d2 = fmaf(u2, u2, fmaf(u1, u1, u0 * u0));
      float v = d2;  // box: the squared distance, turned into the one-hot row below
      if (a.kind != SE3_PNE_KP_BOX) {
        const float tt = sqrtf(d2) / a.sigma;
        v = a.kind == SE3_PNE_KP_GAUSS ? expf(-(tt * tt) * 0.5f) : fmaxf(1.0f - tt, 0.0f);
      }
      in[j][le] = live ? v : 0.f;
    }
    if (a.kind == SE3_PNE_KP_BOX) {
      __syncthreads();
      if (part == 0) {  // the column of this edge belongs to this thread alone
        int best = 0;
        float bd = in[0][le];
        for (int j = 1; j < a.n_in; ++j) {
          const float d = in[j][le];
          if (d < bd) bd = d, best = j;
        }
        for (int j = 0; j < a.n_in; ++j) in[j][le] = (live && j == best) ? 1.0f : 0.0f;
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float pre_activation(const EmbedArgs& a, const float (*in)[kTile], int le, int k) {
  float z = a.beta[k];
  for (int j = 0; j < a.n_in; ++j) z = fmaf(in[j][le], a.A[j * a.k + k], z);
  return z;
}

// softmax: the maximum and the sum of a tile's rows, one thread per edge.  Ends with a barrier.
__device__ __forceinline__ void tile_softmax_stats(const EmbedArgs& a, const float (*in)[kTile], float* row_max, float* row_sum) {
  const int t = threadIdx.x;
  if (t < kTile) {
    float m = pre_activation(a, in, t, 0);
    for (int k = 1; k < a.k; ++k) m = fmaxf(m, pre_activation(a, in, t, k));
    float s = 0.f;
    for (int k = 0; k < a.k; ++k) s += expf(pre_activation(a, in, t, k) - m);
    row_max[t] = m, row_sum[t] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ float activation(int kind, float z, float m, float s) {
  switch (kind) {
    case SE3_PNE_MLP_RELU: return fmaxf(z, 0.f);
    case SE3_PNE_MLP_GELU: return 0.5f * z * (1.0f + erff(z * 0.70710678118654752440f));
    case SE3_PNE_MLP_SIN: return sinf(z);
    case SE3_PNE_MLP_SOFTMAX: return expf(z - m) / s;
    default: return z;
  }
}

// gz of one value (softmax: `q` is the row's sum of g * phi)
__device__ __forceinline__ float chain(int kind, float z, float g, float m, float s, float q) {
  switch (kind) {
    case SE3_PNE_MLP_RELU: return z > 0.f ? g : 0.f;
    case SE3_PNE_MLP_GELU: {
      const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
      const float pdf = expf(-(z * z) * 0.5f) * 0.39894228040143267794f;
      return g * fmaf(z, pdf, cdf);
    }
    case SE3_PNE_MLP_SIN: return g * cosf(z);
    case SE3_PNE_MLP_SOFTMAX: return (expf(z - m) / s) * (g - q);
    default: return g;
  }
}

__global__ __launch_bounds__(kThreads) void pne_embed_fwd_kernel(EmbedArgs a, float* __restrict__ phi) {
  __shared__ float in[kMaxIn][kTile];
  __shared__ float row_max[kTile], row_sum[kTile];
  const int e0 = blockIdx.x * kTile;
  tile_inputs(a, e0, in);
  const bool softmax = a.kind == SE3_PNE_MLP_SOFTMAX;
  if (softmax) tile_softmax_stats(a, in, row_max, row_sum);
  const int rows = min(kTile, a.e_total - e0);
  const int n = rows * a.k;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int le = i / a.k, k = i - le * a.k;
    const float z = pre_activation(a, in, le, k);
    phi[(size_t)e0 * a.k + i] = activation(a.kind, z, softmax ? row_max[le] : 0.f, softmax ? row_sum[le] : 1.f);
  }
}

// partials [chunk][n_in + 1][K] (row n_in: dbeta)
__global__ __launch_bounds__(kThreads) void pne_embed_bwd_chunks_kernel(EmbedArgs a, const float* __restrict__ grad_phi,
                                                                        double* __restrict__ partials) {
  __shared__ float in[kMaxIn][kTile];
  __shared__ float gz[kTile][kSlab + 1];
  __shared__ float row_max[kTile], row_sum[kTile], row_q[kTile];
  const int t = threadIdx.x;
  const int c0 = blockIdx.x * SE3_PNE_CHUNK;
  const int c1 = min(c0 + SE3_PNE_CHUNK, a.e_total);
  const bool softmax = a.kind == SE3_PNE_MLP_SOFTMAX;
  const int rows_in = a.n_in + 1;
  double* mine = partials + (size_t)blockIdx.x * rows_in * a.k;
  for (int k0 = 0; k0 < a.k; k0 += kSlab) {
    const int kn = min(kSlab, a.k - k0);
    const int pairs = rows_in * kn;
    double acc[kPairs];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) acc[p] = 0.0;
    for (int e0 = c0; e0 < c1; e0 += kTile) {
      __syncthreads();  // the previous tile's LDS has been read
      tile_inputs(a, e0, in);
      if (softmax) {
        tile_softmax_stats(a, in, row_max, row_sum);
        if (t < kTile) {
          float q = 0.f;
          if (e0 + t < c1)
            for (int k = 0; k < a.k; ++k)
              q = fmaf(grad_phi[(size_t)(e0 + t) * a.k + k], expf(pre_activation(a, in, t, k) - row_max[t]) / row_sum[t], q);
          row_q[t] = q;
        }
        __syncthreads();
      }
      const int rows = min(kTile, c1 - e0);
      for (int i = t; i < kTile * kn; i += kThreads) {
        const int le = i / kn, kk = i - le * kn;
        float v = 0.f;  // an absent edge of the last tile adds +0.0: an exact identity (a partial is never -0.0)
        if (le < rows) {
          const float z = is_kp(a.kind) || a.kind == SE3_PNE_MLP_LINEAR ? 0.f : pre_activation(a, in, le, k0 + kk);
          v = chain(a.kind, z, grad_phi[(size_t)(e0 + le) * a.k + k0 + kk], softmax ? row_max[le] : 0.f,
                    softmax ? row_sum[le] : 1.f, softmax ? row_q[le] : 0.f);
        }
        gz[le][kk] = v;
      }
      __syncthreads();
#pragma unroll
      for (int p = 0; p < kPairs; ++p) {
        const int i = t + p * kThreads;
        if (i < pairs) {
          const int j = i / kn, kk = i - j * kn;
          double s = acc[p];
          if (j < a.n_in) {
            for (int le = 0; le < rows; ++le) s += (double)in[j][le] * (double)gz[le][kk];
          } else {
            for (int le = 0; le < rows; ++le) s += (double)gz[le][kk];
          }
          acc[p] = s;
        }
      }
    }
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
      const int i = t + p * kThreads;
      if (i < pairs) {
        const int j = i / kn, kk = i - j * kn;
        mine[(size_t)j * a.k + k0 + kk] = acc[p];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void pne_embed_bwd_finish_kernel(const double* __restrict__ partials, int chunks, int n_in,
                                                                        int k, float* __restrict__ dA, float* __restrict__ dbeta) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int total = (n_in + 1) * k;
  if (i >= total) return;
  double s = 0.0;
  for (int c0 = 0; c0 < chunks; c0 += kAhead) {  // the additions are a serial chain in ascending c; the loads are not
    double part[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) part[u] = c0 + u < chunks ? partials[(size_t)(c0 + u) * total + i] : 0.0;
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
      if (c0 + u < chunks) s += part[u];
  }
  if (i < n_in * k) dA[i] = (float)s;
  else dbeta[i - n_in * k] = (float)s;
}

// ------------------------------------------------------------------------------------------------------ max aggregation
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(kThreads) void neigh_max_fwd_kernel(const float* __restrict__ phi, const float* __restrict__ G,
                                                                 const int32_t* __restrict__ neighbors,
                                                                 const int32_t* __restrict__ ends, int n_samples, int k, int c,
                                                                 float* __restrict__ out, int32_t* __restrict__ arg) {
  const int m = wave_uniform(blockIdx.x * (kThreads / kWave) + (int)(threadIdx.x / kWave));
  if (m >= n_samples) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int e_begin = m > 0 ? ends[m - 1] : 0, e_end = ends[m];
  for (int o0 = 0; o0 < c; o0 += kWave) {
    const int o = o0 + lane;
    const bool live = o < c;
    float best = 0.f;
    int best_e = -1;
    for (int e = e_begin; e < e_end; ++e) {
      const int src = neighbors[2 * e + 1];
      const float* g = G + (size_t)src * k * c + (live ? o : 0);
      const float* p = phi + (size_t)e * k;
      float v = 0.f;
      int kk = 0;
      for (; kk + kAhead <= k; kk += kAhead) {  // the rows of G kAhead at a time: their loads are in flight together
        float row[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) row[u] = g[(size_t)(kk + u) * c];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v = fmaf(p[kk + u], row[u], v);
      }
      for (; kk < k; ++kk) v = fmaf(p[kk], g[(size_t)kk * c], v);
      if (best_e < 0 || v > best) best = v, best_e = e;
    }
    if (live) out[(size_t)m * c + o] = best, arg[(size_t)m * c + o] = best_e;
  }
}

__global__ __launch_bounds__(kThreads) void neigh_max_dphi_kernel(const float* __restrict__ grad_out, const int32_t* __restrict__ arg,
                                                                  const float* __restrict__ G, const int32_t* __restrict__ neighbors,
                                                                  const int32_t* __restrict__ ends, int n_samples, int k, int c,
                                                                  float* dphi) {
  const int m = wave_uniform(blockIdx.x * (kThreads / kWave) + (int)(threadIdx.x / kWave));
  if (m >= n_samples) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int e_begin = m > 0 ? ends[m - 1] : 0, e_end = ends[m];
  for (int kk = lane; kk < k; kk += kWave) {  // lane `kk % 64` owns column kk of every row of this sample
    for (int e = e_begin; e < e_end; ++e) dphi[(size_t)e * k + kk] = 0.f;
    // kGroup channels at a time: their winners, gradients, rows of G and of dphi are loaded together, the sums are formed
    // in ascending o in registers -- a later channel of the group with the same winner takes up the earlier one's sum -- and
    // every row is stored once, by its last channel of the group, before the next group loads.
    for (int o0 = 0; o0 < c; o0 += kGroup) {
      int e[kGroup];
      float g[kGroup], gv[kGroup], d[kGroup];
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        const int o = o0 + u;
        e[u] = o < c ? arg[(size_t)m * c + o] : -1;
        if (e[u] < e_begin || e[u] >= e_end) e[u] = -1;  // (-1 of an empty sample, or nothing the forward call wrote)
        g[u] = e[u] >= 0 ? grad_out[(size_t)m * c + o] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        const int src = e[u] >= 0 ? neighbors[2 * e[u] + 1] : 0;
        gv[u] = e[u] >= 0 ? G[((size_t)src * k + kk) * c + o0 + u] : 0.f;
        d[u] = e[u] >= 0 ? dphi[(size_t)e[u] * k + kk] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        if (e[u] < 0) continue;
#pragma unroll
        for (int v = 0; v < u; ++v)
          if (e[v] == e[u]) d[u] = d[v];  // ascending v: the latest earlier sum of the same row wins
        d[u] = fmaf(g[u], gv[u], d[u]);
      }
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        bool last = e[u] >= 0;
#pragma unroll
        for (int v = u + 1; v < kGroup; ++v) last = last && e[v] != e[u];
        if (last) dphi[(size_t)e[u] * k + kk] = d[u];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void neigh_max_dg_kernel(const float* __restrict__ grad_out, const int32_t* __restrict__ arg,
                                                                const float* __restrict__ phi, const int32_t* __restrict__ t_samples,
                                                                const int32_t* __restrict__ t_ends,
                                                                const int32_t* __restrict__ t_edge_ids, int n_src, int k, int c,
                                                                int o_tiles, float* __restrict__ dG) {
  const int w = wave_uniform(blockIdx.x * (kThreads / kWave) + (int)(threadIdx.x / kWave));
  if (w >= n_src * o_tiles) return;
  const int p = w / o_tiles, o = (w - p * o_tiles) * kWave + (int)(threadIdx.x & (kWave - 1));
  const bool live = o < c;
  const int i_begin = p > 0 ? t_ends[p - 1] : 0, i_end = t_ends[p];
  for (int k0 = 0; k0 < k; k0 += kSlab) {
    const int kn = min(kSlab, k - k0);
    float acc[kSlab];
#pragma unroll
    for (int kk = 0; kk < kSlab; ++kk) acc[kk] = 0.f;
    for (int i = i_begin; i < i_end; ++i) {
      const int m = t_samples[i], e = t_edge_ids[i];
      const bool win = live && arg[(size_t)m * c + o] == e;
      if (__ballot(win) == 0) continue;
      const float g = win ? grad_out[(size_t)m * c + o] : 0.f;
      const float* ph = phi + (size_t)e * k + k0;
      if (win) {
#pragma unroll
        for (int kk = 0; kk < kSlab; ++kk)
          if (kk < kn) acc[kk] = fmaf(g, ph[kk], acc[kk]);
      }
    }
    if (live) {
#pragma unroll
      for (int kk = 0; kk < kSlab; ++kk)
        if (kk < kn) dG[((size_t)p * k + k0 + kk) * c + o] = acc[kk];
    }
  }
}

constexpr int64_t kLim = 1ll << 31;
inline bool beyond(int64_t a, int64_t b) { return a > 0 && b > 0 && a >= (kLim + b - 1) / b; }  // a * b >= 2^31, no overflow

int embed_shape(int64_t n_edges, int32_t kind, int32_t n_kpts, int32_t num_basis) {
  if (n_edges < 0 || num_basis < 1 || kind < SE3_PNE_MLP_LINEAR || kind > SE3_PNE_KP_BOX) return SE3_ERR_INVALID_ARGUMENT;
  if (is_kp(kind) && n_kpts < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (is_kp(kind) && n_kpts > SE3_PNE_MAX_KPTS) return SE3_ERR_UNSUPPORTED;
  if (beyond(n_edges, num_basis) || beyond(n_edges, 2) || beyond(inputs_of(kind, n_kpts) + 1, num_basis)) return SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}

int64_t chunks_of(int64_t n_edges) { return (n_edges + SE3_PNE_CHUNK - 1) / SE3_PNE_CHUNK; }

size_t embed_workspace(int64_t n_edges, int32_t kind, int32_t n_kpts, int32_t num_basis) {
  const size_t chunks = (size_t)(n_edges > 0 ? chunks_of(n_edges) : 1);
  return align_up(chunks * (size_t)(inputs_of(kind, n_kpts) + 1) * (size_t)num_basis * sizeof(double), 256);
}

int embed_pointers(int64_t n_edges, int32_t kind, const float* pts, const float* samples, const int32_t* neighbors,
                   const float* rho, const float* kpts, float sigma, const float* A, const float* beta) {
  if (!rho || !A || !beta) return SE3_ERR_INVALID_ARGUMENT;
  if (is_kp(kind) && (!kpts || !(sigma > 0.f) || !(sigma < __builtin_inff()))) return SE3_ERR_INVALID_ARGUMENT;
  if (n_edges > 0 && (!pts || !samples || !neighbors)) return SE3_ERR_INVALID_ARGUMENT;
  return SE3_OK;
}

int max_shape(int64_t n_edges, int64_t n_samples, int64_t n_src, int32_t num_basis, int32_t c_out) {
  if (n_edges < 0 || n_samples < 0 || n_src < 0 || num_basis < 1 || c_out < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (beyond(n_edges, num_basis) || beyond(n_edges, 2) || beyond(n_samples, c_out) || beyond(num_basis, c_out) ||
      beyond(n_src, (int64_t)num_basis * c_out))
    return SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + kThreads - 1) / kThreads); }

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" size_t se3_pne_embed_workspace_bytes(int64_t n_edges, int32_t kind, int32_t n_kpts, int32_t num_basis) {
  if (embed_shape(n_edges, kind, n_kpts, num_basis) != SE3_OK) return 0;
  return embed_workspace(n_edges, kind, n_kpts, num_basis);
}

extern "C" int se3_pne_embed_fwd(const float* pts, const float* samples, const int32_t* neighbors, int64_t n_edges,
                                 const float* rho, int32_t kind, const float* kpts, int32_t n_kpts, float sigma, const float* A,
                                 const float* beta, int32_t num_basis, float* phi, void* stream_) {
  if (int rc = embed_shape(n_edges, kind, n_kpts, num_basis)) return rc;
  if (int rc = embed_pointers(n_edges, kind, pts, samples, neighbors, rho, kpts, sigma, A, beta)) return rc;
  if (n_edges == 0) return SE3_OK;
  if (!phi) return SE3_ERR_INVALID_ARGUMENT;
  const EmbedArgs a{pts, samples, neighbors, rho, kpts, A, beta, (int)n_edges, kind, inputs_of(kind, n_kpts), num_basis, sigma};
  hipLaunchKernelGGL(pne_embed_fwd_kernel, dim3((unsigned)((n_edges + kTile - 1) / kTile)), dim3(kThreads), 0,
                     (hipStream_t)stream_, a, phi);
  return check_launch();
}

extern "C" int se3_pne_embed_bwd(const float* grad_phi, const float* pts, const float* samples, const int32_t* neighbors,
                                 int64_t n_edges, const float* rho, int32_t kind, const float* kpts, int32_t n_kpts, float sigma,
                                 const float* A, const float* beta, int32_t num_basis, float* dA, float* dbeta, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  if (int rc = embed_shape(n_edges, kind, n_kpts, num_basis)) return rc;
  if (int rc = embed_pointers(n_edges, kind, pts, samples, neighbors, rho, kpts, sigma, A, beta)) return rc;
  if (!dA || !dbeta || !workspace || (n_edges > 0 && !grad_phi)) return SE3_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < embed_workspace(n_edges, kind, n_kpts, num_basis)) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int n_in = inputs_of(kind, n_kpts);
  const int chunks = (int)chunks_of(n_edges);
  double* partials = (double*)workspace;
  if (chunks > 0) {
    const EmbedArgs a{pts, samples, neighbors, rho, kpts, A, beta, (int)n_edges, kind, n_in, num_basis, sigma};
    hipLaunchKernelGGL(pne_embed_bwd_chunks_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, stream, a, grad_phi, partials);
  }
  hipLaunchKernelGGL(pne_embed_bwd_finish_kernel, dim3(blocks_of((int64_t)(n_in + 1) * num_basis)), dim3(kThreads), 0, stream,
                     partials, chunks, n_in, num_basis, dA, dbeta);
  return check_launch();
}

extern "C" int se3_neigh_max_fwd(const float* phi, const float* G, const int32_t* neighbors, const int32_t* ends,
                                 int64_t n_edges, int64_t n_samples, int64_t n_src, int32_t num_basis, int32_t c_out, float* out,
                                 int32_t* arg, void* stream_) {
  if (int rc = max_shape(n_edges, n_samples, n_src, num_basis, c_out)) return rc;
  if (n_samples == 0) return SE3_OK;
  if (!out || !arg || !ends || (n_edges > 0 && (!phi || !G || !neighbors))) return SE3_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(neigh_max_fwd_kernel, dim3(blocks_of(n_samples * kWave)), dim3(kThreads), 0, (hipStream_t)stream_, phi, G,
                     neighbors, ends, (int)n_samples, num_basis, c_out, out, arg);
  return check_launch();
}

extern "C" int se3_neigh_max_bwd(const float* grad_out, const int32_t* arg, const float* phi, const float* G,
                                 const int32_t* neighbors, const int32_t* ends, const int32_t* t_samples, const int32_t* t_ends,
                                 const int32_t* t_edge_ids, int64_t n_edges, int64_t n_samples, int64_t n_src, int32_t num_basis,
                                 int32_t c_out, float* dphi, float* dG, void* stream_) {
  if (int rc = max_shape(n_edges, n_samples, n_src, num_basis, c_out)) return rc;
  if ((n_samples > 0 && (!grad_out || !arg || !ends)) || (n_src > 0 && (!dG || !t_ends)) ||
      (n_edges > 0 && (!phi || !G || !neighbors || !t_samples || !t_edge_ids || !dphi)))
    return SE3_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  if (n_samples > 0 && n_edges > 0)
    hipLaunchKernelGGL(neigh_max_dphi_kernel, dim3(blocks_of(n_samples * kWave)), dim3(kThreads), 0, stream, grad_out, arg, G,
                       neighbors, ends, (int)n_samples, num_basis, c_out, dphi);
  if (n_src > 0) {
    const int o_tiles = (c_out + kWave - 1) / kWave;
    hipLaunchKernelGGL(neigh_max_dg_kernel, dim3(blocks_of(n_src * o_tiles * kWave)), dim3(kThreads), 0, stream, grad_out, arg, phi,
                       t_samples, t_ends, t_edge_ids, (int)n_src, num_basis, c_out, o_tiles, dG);
  }
  return check_launch();
}
