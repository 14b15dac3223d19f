// ElasticDistortionAug for gfx950 (include/se3conv_elastic.h holds the contract; replaces the conv3d + grid_sample of
// point_cloud_lib/augment/ElasticDistortionAug.py, which the reference runs on one scene at a time on the host).
//
//   elastic_plan_kernel      one workgroup: dims per (element, octave), then ONE thread's prefix over the entries: offsets,
//                            the overflow word, the tile prefix
//   elastic_grids_kernel     kGridBlocks resident workgroups stride over the tile count the plan left.  Per tile of T^3 cells:
//                            (T+4)^3 x 3 raw numbers from the hash (or from noise_in) into LDS, six blur passes between two
//                            LDS images on shrinking regions, one 16-byte store per cell
//   elastic_displace_kernel  one thread per row: the octaves in turn, 8 16-byte corner loads each
//
// LDS of the blur: 2 images x 3 channels x 12^3 floats = 41 472 bytes, three workgroups of 256 threads per CU.  Every pass
// walks its region with the z index fastest across the lanes of a wavefront, whatever the pass's axis: a lane reads its own
// cell and the two at -stride / +stride, so the 64 lanes of each of the three reads touch runs of consecutive words (runs of
// 8 to 12, the region's z edge) and no pass direction is a strided, bank-conflicting walk.  Contraction is off for the whole
// file; nothing adds floating-point numbers with atomics and no workgroup waits for another.
#include "common.h"
#include "../../include/se3conv_augment.h"
#include "../../include/se3conv_elastic.h"

#pragma clang fp contract(off)

namespace se3 {

namespace {

constexpr int kDraws = SE3_AUG_DRAWS;
constexpr int kMaxOct = SE3_ELASTIC_MAX_OCTAVES;
constexpr int kTile = SE3_ELASTIC_TILE;
constexpr int kHalo = 2;                    // two blur passes per axis
constexpr int kEdge = kTile + 2 * kHalo;    // 12
constexpr int kEdge3 = kEdge * kEdge * kEdge;
constexpr int kGridThreads = 256;
constexpr int kGridBlocks = 1024;           // resident: 256 CUs x 3 workgroups fit 768 at a time, the rest queue behind them
constexpr float kThird = 0.3333333432674407958984375f;  // fp32(1/3)

struct ElasticConsts {
  float v[kMaxOct];
};

__device__ __forceinline__ uint32_t el_mix(uint32_t x) {
  x ^= x >> 16, x *= 0x85ebca6bu, x ^= x >> 13, x *= 0xc2b2ae35u, x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t el_h(uint32_t seed, uint32_t s, uint32_t p) { return el_mix(el_mix(seed ^ el_mix(s)) + p * 0x9E3779B9u); }
__device__ __forceinline__ uint32_t el_word(uint32_t key, uint32_t j) { return el_mix(key + (j + 1u) * 0x9E3779B9u); }
__device__ __forceinline__ float el_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }  // 2^-24: exact

__device__ __forceinline__ int64_t el_tiles(int64_t n) { return (n + kTile - 1) / kTile; }

// ------------------------------------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(256) void elastic_plan_kernel(const int32_t* __restrict__ counts, const float* __restrict__ stats,
                                                           const float* __restrict__ draws, float prob, ElasticConsts g,
                                                           int32_t n_octaves, int32_t n_batches, int64_t capacity,
                                                           int64_t* table, int32_t* __restrict__ overflow,
                                                           int64_t* __restrict__ tile_prefix) {
  for (int b = threadIdx.x; b < n_batches; b += 256) {
    const bool open = draws[(int64_t)b * kDraws] <= prob && counts[b] > 0;
    int64_t n[kMaxOct][3];
    bool finite = open;
    if (open) {
      const float* st = stats + (int64_t)b * 12;
      for (int l = 0; l < n_octaves; ++l)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float q = (st[3 + j] - st[j]) / g.v[l];
          const bool ok = q >= 0.f && q < (float)SE3_ELASTIC_MAX_QUOTIENT;
          finite = finite && ok;
          n[l][j] = ok ? (int64_t)((int)floorf(q) + 3) : 0;
        }
    }
    for (int l = 0; l < n_octaves; ++l) {
      int64_t* e = table + ((int64_t)b * n_octaves + l) * 4;
#pragma unroll
      for (int j = 0; j < 3; ++j) e[j] = finite ? n[l][j] : 0;
      e[3] = -1;
    }
  }
  __syncthreads();  // (the table words above are read back by thread 0 of this same workgroup)
  if (threadIdx.x != 0) return;
  int64_t off = 0, tiles = 0;
  int32_t flag = 0;
  bool full = false;
  for (int b = 0; b < n_batches; ++b) {
    int64_t* e = table + (int64_t)b * n_octaves * 4;
    const bool open = draws[(int64_t)b * kDraws] <= prob && counts[b] > 0;
    bool distorted = false;
    if (open && e[0] == 0) flag |= 2;  // (an open, finite element has dims >= 3)
    if (open && e[0] != 0) {
      int64_t o = off;
      bool fits = !full;
      for (int l = 0; l < n_octaves && fits; ++l) {
        const int64_t cells = e[4 * l] * e[4 * l + 1] * e[4 * l + 2];  // < 2^61
        if (cells > capacity - o) fits = false;
        else o += cells;
      }
      if (fits) {
        distorted = true;
        for (int l = 0; l < n_octaves; ++l) {
          e[4 * l + 3] = off;
          off += e[4 * l] * e[4 * l + 1] * e[4 * l + 2];
        }
      } else {
        flag |= 1, full = true;
      }
    }
    for (int l = 0; l < n_octaves; ++l) {
      tile_prefix[(int64_t)b * n_octaves + l] = tiles;
      if (distorted) tiles += el_tiles(e[4 * l]) * el_tiles(e[4 * l + 1]) * el_tiles(e[4 * l + 2]);
    }
  }
  tile_prefix[(int64_t)n_batches * n_octaves] = tiles;
  overflow[0] = flag;
}

// ----------------------------------------------------------------------------------------------------------------- grids
__global__ __launch_bounds__(kGridThreads) void elastic_grids_kernel(const int64_t* __restrict__ table,
                                                                     const int64_t* __restrict__ tile_prefix, int32_t n_entries,
                                                                     int32_t n_octaves, uint32_t seed,
                                                                     const uint32_t* __restrict__ seed_device, uint32_t step,
                                                                     const float* __restrict__ noise_in, float* __restrict__ grid) {
  __shared__ float buf[2][3 * kEdge3];
  const int t = threadIdx.x;
  const int64_t total = tile_prefix[n_entries];
  const uint32_t seed_eff = seed + (seed_device ? *seed_device : 0u);
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {  // (uniform per workgroup)
    int e0 = 0, e1 = n_entries + 1;  // the last entry with tile_prefix[e] <= tile: entries without tiles are passed over
    while (e0 < e1) {
      const int mid = e0 + ((e1 - e0) >> 1);
      if (tile_prefix[mid] <= tile) e0 = mid + 1;
      else e1 = mid;
    }
    const int e = e0 - 1;
    const int64_t* ent = table + (int64_t)e * 4;
    const int nx = (int)ent[0], ny = (int)ent[1], nz = (int)ent[2];
    const int64_t off = ent[3];
    const int64_t local = tile - tile_prefix[e], ty_n = el_tiles(ny), tz_n = el_tiles(nz);
    const int x0 = (int)(local / (ty_n * tz_n)) * kTile - kHalo, y0 = (int)((local / tz_n) % ty_n) * kTile - kHalo,
              z0 = (int)(local % tz_n) * kTile - kHalo;
    const uint32_t seed_bl = el_h(seed_eff, step, (uint32_t)((e / n_octaves) * kMaxOct + e % n_octaves));
    // the raw numbers of the tile and its halo
    for (int i = t; i < kEdge3; i += kGridThreads) {
      const int gx = x0 + i / (kEdge * kEdge), gy = y0 + (i / kEdge) % kEdge, gz = z0 + i % kEdge;
      float v[3] = {0.f, 0.f, 0.f};
      if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) {
        const int64_t q = ((int64_t)gx * ny + gy) * nz + gz;
        if (noise_in) {
          const float4 r = reinterpret_cast<const float4*>(noise_in)[off + q];
          v[0] = r.x, v[1] = r.y, v[2] = r.z;
        } else {
          const uint32_t key = el_h(seed_bl, 0u, (uint32_t)q);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float u1 = el_uniform(el_word(key, 2 * c)), u2 = el_uniform(el_word(key, 2 * c + 1));
            v[c] = sqrtf(-2.f * logf(1.f - u1)) * cosf(6.283185307179586f * u2);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) buf[0][c * kEdge3 + i] = v[c];
    }
    __syncthreads();
    // six passes; pass p blurs along axis p % 3 and leaves axis j valid on [s_j, kEdge - s_j), s_j = passes along j so far
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int a = p % 3;
      const int sx = (p >= 0) + (p >= 3), sy = (p >= 1) + (p >= 4), sz = (p >= 2) + (p >= 5);
      const int rx = kEdge - 2 * sx, ry = kEdge - 2 * sy, rz = kEdge - 2 * sz;
      const int stride = a == 0 ? kEdge * kEdge : a == 1 ? kEdge : 1;
      const float* __restrict__ src = buf[p & 1];
      float* __restrict__ dst = buf[(p & 1) ^ 1];
      const int cells = rx * ry * rz;
      for (int i = t; i < 3 * cells; i += kGridThreads) {
        const int c = i / cells, r = i - c * cells;
        const int lx = sx + r / (ry * rz), ly = sy + (r / rz) % ry, lz = sz + r % rz;
        const int at = c * kEdge3 + (lx * kEdge + ly) * kEdge + lz;
        const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
        const bool inside = gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz;
        dst[at] = inside ? ((src[at - stride] * kThird) + (src[at] * kThird)) + (src[at + stride] * kThird) : 0.f;
      }
      __syncthreads();
    }
    // (six passes: the result stands in buf[0], valid on [kHalo, kHalo + kTile)^3)
    for (int i = t; i < kTile * kTile * kTile; i += kGridThreads) {
      const int lx = kHalo + i / (kTile * kTile), ly = kHalo + (i / kTile) % kTile, lz = kHalo + i % kTile;
      const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
      if (gx < nx && gy < ny && gz < nz) {  // (>= 0: the tile itself starts inside the grid)
        const int at = (lx * kEdge + ly) * kEdge + lz;
        const int64_t q = ((int64_t)gx * ny + gy) * nz + gz;
        reinterpret_cast<float4*>(grid)[off + q] = make_float4(buf[0][at], buf[0][kEdge3 + at], buf[0][2 * kEdge3 + at], 0.f);
      }
    }
    __syncthreads();  // buf[0] is the next tile's raw image
  }
}

// -------------------------------------------------------------------------------------------------------------- displace
__global__ __launch_bounds__(256) void elastic_displace_kernel(const float* __restrict__ x, const int32_t* __restrict__ batch_ids,
                                                               int64_t n_rows, const int32_t* __restrict__ n_valid, int32_t n_batches,
                                                               const float* __restrict__ stats, const int64_t* __restrict__ table,
                                                               int32_t n_octaves, ElasticConsts m, const float* __restrict__ grid,
                                                               float* __restrict__ y) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  float c[3] = {0.f, 0.f, 0.f};
  if (r < present_rows(n_valid, n_rows)) {
    c[0] = x[r * 3], c[1] = x[r * 3 + 1], c[2] = x[r * 3 + 2];
    const int b = batch_ids[r];
    if (b >= 0 && b < n_batches && table[(int64_t)b * n_octaves * 4 + 3] >= 0) {
      const float* st = stats + (int64_t)b * 12;
      const float lo[3] = {st[0], st[1], st[2]}, hi[3] = {st[3], st[4], st[5]};
      for (int l = 0; l < n_octaves; ++l) {
        const int64_t* ent = table + ((int64_t)b * n_octaves + l) * 4;
        const int n[3] = {(int)ent[0], (int)ent[1], (int)ent[2]};
        const float4* g = reinterpret_cast<const float4*>(grid) + ent[3];
        int i[3];
        float f[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float top = (float)(n[j] - 1);
          float p = hi[j] == lo[j] ? 0.f : ((c[j] - lo[j]) / (hi[j] - lo[j])) * top;
          p = fminf(fmaxf(p, 0.f), top);
          i[j] = min((int)floorf(p), n[j] - 2);
          f[j] = p - (float)i[j];
        }
        float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
          const float w = ((dx ? f[0] : 1.f - f[0]) * (dy ? f[1] : 1.f - f[1])) * (dz ? f[2] : 1.f - f[2]);
          const float4 v = g[((int64_t)(i[0] + dx) * n[1] + (i[1] + dy)) * n[2] + (i[2] + dz)];
          s[0] = s[0] + w * v.x, s[1] = s[1] + w * v.y, s[2] = s[2] + w * v.z;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = c[j] + s[j] * m.v[l];
      }
    }
  }
  y[r * 3] = c[0], y[r * 3 + 1] = c[1], y[r * 3 + 2] = c[2];
}

inline size_t elastic_workspace(int32_t n_batches, int32_t n_octaves) {
  return align_up(sizeof(int64_t) * ((size_t)n_batches * (size_t)n_octaves + 1), 256);
}
inline bool octaves_ok(int32_t n_octaves) { return n_octaves >= 1 && n_octaves <= kMaxOct; }

}  // namespace

}  // namespace se3

using namespace se3;

extern "C" size_t se3_elastic_workspace_bytes(int32_t n_batches, int32_t n_octaves) {
  if (n_batches < 1 || !octaves_ok(n_octaves)) return 0;
  return elastic_workspace(n_batches, n_octaves);
}

extern "C" int se3_elastic_plan(const int32_t* counts, const float* stats, const float* draws, float prob, const double* granularity,
                                int32_t n_octaves, int32_t n_batches, int64_t grid_capacity, int64_t* grid_table, int32_t* overflow,
                                void* workspace, size_t workspace_bytes, void* stream_) {
  if (n_batches < 1 || !octaves_ok(n_octaves) || grid_capacity < 0) return SE3_ERR_INVALID_ARGUMENT;
  if (!counts || !stats || !draws || !granularity || !grid_table || !overflow || !workspace) return SE3_ERR_INVALID_ARGUMENT;
  ElasticConsts g = {};
  for (int l = 0; l < n_octaves; ++l) {
    g.v[l] = (float)granularity[l];
    if (!(g.v[l] > 0.f)) return SE3_ERR_INVALID_ARGUMENT;
  }
  if (workspace_bytes < elastic_workspace(n_batches, n_octaves)) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope prof("elastic_plan", stream);
  hipLaunchKernelGGL(elastic_plan_kernel, dim3(1), dim3(256), 0, stream, counts, stats, draws, prob, g, n_octaves, n_batches, grid_capacity,
                     grid_table, overflow, (int64_t*)workspace);
  return check_launch();
}

extern "C" int se3_elastic_grids(const int64_t* grid_table, int32_t n_batches, int32_t n_octaves, int64_t grid_capacity, uint32_t seed,
                                 const uint32_t* seed_device, uint32_t step, const float* noise_in, float* grid, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  if (n_batches < 1 || !octaves_ok(n_octaves) || grid_capacity < 0) return SE3_ERR_INVALID_ARGUMENT;
  if (!grid_table || !workspace || (grid_capacity > 0 && !grid)) return SE3_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < elastic_workspace(n_batches, n_octaves)) return SE3_ERR_WORKSPACE;
  if ((int64_t)n_batches * n_octaves >= (int64_t)1 << 31) return SE3_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope prof("elastic_grids", stream);
  hipLaunchKernelGGL(elastic_grids_kernel, dim3(kGridBlocks), dim3(kGridThreads), 0, stream, grid_table, (const int64_t*)workspace,
                     n_batches * n_octaves, n_octaves, seed, seed_device, step, noise_in, grid);
  return check_launch();
}

extern "C" int se3_elastic_displace(const float* x, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid, int32_t n_batches,
                                    const float* stats, const int64_t* grid_table, int32_t n_octaves, const double* magnitude,
                                    const float* grid, float* y, void* stream_) {
  if (n_rows < 0 || n_batches < 1 || !octaves_ok(n_octaves)) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows >= (int64_t)1 << 31) return SE3_ERR_UNSUPPORTED;
  if (!stats || !grid_table || !magnitude) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows > 0 && (!x || !batch_ids || !y || !grid)) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return SE3_OK;
  ElasticConsts m = {};
  for (int l = 0; l < n_octaves; ++l) m.v[l] = (float)magnitude[l];
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope prof("elastic_displace", stream);
  hipLaunchKernelGGL(elastic_displace_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream, x, batch_ids, n_rows, n_valid,
                     n_batches, stats, grid_table, n_octaves, m, grid, y);
  return check_launch();
}
