// The augmentation pipeline for gfx950 (include/se3conv_augment.h holds the contract; replaces point_cloud_lib/augment/ of
// the reference, which augments one scene at a time on the host).
//
//   aug_elements_kernel      one workgroup: element boundaries (binary search in the sorted ids) and the first chunk slot of
//                            every element
//   aug_stats_chunk_kernel   one workgroup per chunk of SE3_AUG_CHUNK rows: six fp64 sums by a fixed tree, six fp32 bounds
//   aug_stats_finish_kernel  one workgroup per element: the chunk sums in ascending order, mean and unbiased std
//   aug_affine_step_kernel   one thread per element: the step's (A, s) composed into the table
//   aug_apply_kernel         one thread per row: y = x M + t, hashed Gaussian noise, the rows DropAug sets to one
//   aug_mask_rows_kernel     one thread per row: DropAug and CropBoxAug (and "keep" for CropPtsAug)
//   aug_crop_pts_kernel      one workgroup per element: radix select of the m-th smallest squared distance (4 passes of 8
//                            bits over the distance bits, recomputed every pass: no workspace), ties by row order
//   aug_flags_kernel, hipcub::DeviceScan::ExclusiveSum, aug_compact_kernel      the stable compaction
//
// Nothing here adds floating-point numbers with atomics (the histogram of the radix select counts in integers), no
// workgroup waits for another one, and every product and sum is rounded on its own: contraction is off for the whole file.
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "../../include/se3conv_augment.h"

#pragma clang fp contract(off)

namespace se3 {

namespace {

constexpr int kChunk = SE3_AUG_CHUNK;
constexpr int kDraws = SE3_AUG_DRAWS;
constexpr int kSelThreads = 1024;
constexpr double kPi = 3.141592653589793238462643383279502884;

struct AugConsts {
  double c[SE3_AUG_CONSTS];
};

struct StatsLayout {
  size_t elem_starts, slot_starts, sums, bounds, total;
  int64_t slots;
};
inline StatsLayout stats_layout(int64_t n_rows, int32_t n_batches) {
  StatsLayout l;
  l.slots = (n_rows + kChunk - 1) / kChunk + n_batches;  // >= sum of ceil(n_b / chunk)
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t at = off; off += align_up(bytes, 256); return at; };
  l.elem_starts = take(sizeof(int32_t) * ((size_t)n_batches + 1));
  l.slot_starts = take(sizeof(int32_t) * ((size_t)n_batches + 1));
  l.sums = take(sizeof(double) * 6 * (size_t)l.slots);
  l.bounds = take(sizeof(float) * 6 * (size_t)l.slots);
  l.total = off;
  return l;
}

// first position in ids[0, n) whose value is >= v (ids non-decreasing)
__device__ __forceinline__ int aug_lower_bound(const int32_t* __restrict__ ids, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t aug_mix(uint32_t x) {
  x ^= x >> 16, x *= 0x85ebca6bu, x ^= x >> 13, x *= 0xc2b2ae35u, x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t aug_row_key(uint32_t seed_eff, uint32_t step, uint32_t row) {
  return aug_mix(aug_mix(seed_eff ^ aug_mix(step)) + row * 0x9E3779B9u);
}
__device__ __forceinline__ uint32_t aug_word(uint32_t key, uint32_t j) { return aug_mix(key + (j + 1u) * 0x9E3779B9u); }
__device__ __forceinline__ float aug_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }  // 2^-24: exact
__device__ __forceinline__ uint32_t aug_seed(uint32_t seed, const uint32_t* __restrict__ seed_device) {
  return seed + (seed_device ? *seed_device : 0u);
}

// y = x M + t of the contract (m: the element's twelve words, NULL = identity)
__device__ __forceinline__ void aug_transform(const float* __restrict__ m, bool with_t, const float x[3], float y[3]) {
  if (!m) {
    y[0] = x[0], y[1] = x[1], y[2] = x[2];
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float v = ((x[0] * m[j]) + (x[1] * m[3 + j])) + (x[2] * m[6 + j]);
    y[j] = with_t ? v + m[9 + j] : v;
  }
}

// ------------------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(256) void aug_elements_kernel(const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                           const int32_t* __restrict__ n_valid, int32_t n_batches,
                                                           int32_t* __restrict__ elem_starts, int32_t* __restrict__ slot_starts) {
  const int n = (int)present_rows(n_valid, n_rows);
  for (int b = threadIdx.x; b <= n_batches; b += 256) elem_starts[b] = aug_lower_bound(batch_ids, n, b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int at = 0;
    for (int b = 0; b < n_batches; ++b) {
      slot_starts[b] = at;
      at += (elem_starts[b + 1] - elem_starts[b] + kChunk - 1) / kChunk;
    }
    slot_starts[n_batches] = at;
  }
}

__global__ __launch_bounds__(kChunk) void aug_stats_chunk_kernel(const float* __restrict__ pts, const float* __restrict__ affine,
                                                                 int32_t n_batches, const int32_t* __restrict__ elem_starts,
                                                                 const int32_t* __restrict__ slot_starts,
                                                                 double* __restrict__ sums, float* __restrict__ bounds) {
  __shared__ double sh[6][kChunk];
  __shared__ float lo[3][kChunk], hi[3][kChunk];
  const int64_t slot = blockIdx.x;
  if (slot >= slot_starts[n_batches]) return;  // (uniform)
  int b0 = 0, b1 = n_batches + 1;  // the last b with slot_starts[b] <= slot: the element that owns the slot
  while (b0 < b1) {
    const int mid = b0 + ((b1 - b0) >> 1);
    if (slot_starts[mid] <= slot) b0 = mid + 1;
    else b1 = mid;
  }
  const int b = b0 - 1, t = threadIdx.x;
  const int at = ((int)slot - slot_starts[b]) * kChunk + t, n_b = elem_starts[b + 1] - elem_starts[b];
  float y[3] = {0.f, 0.f, 0.f};
  const bool live = at < n_b;
  if (live) {
    const float* p = pts + (int64_t)(elem_starts[b] + at) * 3;
    const float x[3] = {p[0], p[1], p[2]};
    aug_transform(affine ? affine + (int64_t)b * 12 : nullptr, true, x, y);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double v = (double)y[j];
    sh[j][t] = live ? v : 0.0;
    sh[3 + j][t] = live ? v * v : 0.0;
    lo[j][t] = live ? y[j] : __builtin_inff();
    hi[j][t] = live ? y[j] : -__builtin_inff();
  }
  __syncthreads();
  for (int s = kChunk / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int j = 0; j < 6; ++j) sh[j][t] += sh[j][t + s];
#pragma unroll
      for (int j = 0; j < 3; ++j) lo[j][t] = fminf(lo[j][t], lo[j][t + s]), hi[j][t] = fmaxf(hi[j][t], hi[j][t + s]);
    }
    __syncthreads();
  }
  if (t < 6) sums[slot * 6 + t] = sh[t][0];
  else if (t < 9) bounds[slot * 6 + (t - 6)] = lo[t - 6][0];
  else if (t < 12) bounds[slot * 6 + (t - 6)] = hi[t - 9][0];
}

__global__ __launch_bounds__(64) void aug_stats_finish_kernel(int32_t n_batches, const int32_t* __restrict__ elem_starts,
                                                              const int32_t* __restrict__ slot_starts, const double* __restrict__ sums,
                                                              const float* __restrict__ bounds, int32_t* __restrict__ counts,
                                                              float* __restrict__ stats) {
  __shared__ double tot[6];
  const int b = blockIdx.x, t = threadIdx.x;
  const int s0 = slot_starts[b], s1 = slot_starts[b + 1], n = elem_starts[b + 1] - elem_starts[b];
  if (t < 6) {
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) acc += sums[(int64_t)s * 6 + t];
    tot[t] = acc;
  } else if (t < 12) {
    const bool is_max = t >= 9;
    float acc = is_max ? -__builtin_inff() : __builtin_inff();
    for (int s = s0; s < s1; ++s) {
      const float v = bounds[(int64_t)s * 6 + (t - 6)];
      acc = is_max ? fmaxf(acc, v) : fminf(acc, v);
    }
    stats[(int64_t)b * 12 + (t - 6)] = n > 0 ? acc : 0.f;
  }
  __syncthreads();
  if (t < 3) {
    float mean = 0.f, sd = 0.f;
    if (n > 0) {
      const double dn = (double)n, s1v = tot[t], s2v = tot[3 + t];
      mean = (float)(s1v / dn);
      const double var = (s2v - (s1v * s1v) / dn) / (dn - 1.0);  // n = 1: 0 / 0 = NaN, as torch.std
      sd = (float)sqrt(var < 0.0 ? 0.0 : var);
    }
    stats[(int64_t)b * 12 + 6 + t] = mean;
    stats[(int64_t)b * 12 + 9 + t] = sd;
  }
  if (t == 0) counts[b] = n;
}

// ------------------------------------------------------------------------------------------------------- the affine table
// the reference's three axis matrices, every entry chosen by the axis (no store through an index)
__device__ __forceinline__ void aug_axis_rotation(int axis, double angle, float a[9]) {
  const float c = (float)cos(angle), s = (float)sin(angle);
  a[0] = axis == 0 ? 1.f : c, a[1] = axis == 2 ? -s : 0.f, a[2] = axis == 1 ? s : 0.f;
  a[3] = axis == 2 ? s : 0.f, a[4] = axis == 1 ? 1.f : c, a[5] = axis == 0 ? -s : 0.f;
  a[6] = axis == 1 ? -s : 0.f, a[7] = axis == 0 ? s : 0.f, a[8] = axis == 2 ? 1.f : c;
}

__global__ __launch_bounds__(64) void aug_affine_step_kernel(int32_t kind, AugConsts k, float prob, const float* __restrict__ draws,
                                                             const int32_t* __restrict__ counts, const float* __restrict__ stats,
                                                             int32_t n_batches, float* __restrict__ affine) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n_batches) return;
  const float* u = draws + (int64_t)b * kDraws;
  if (!(u[0] <= prob)) return;
  const float* st = stats ? stats + (int64_t)b * 12 : nullptr;
  float a[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, s[3] = {0.f, 0.f, 0.f};
  switch (kind) {
    case SE3_AUG_ROT_AXIS:
      aug_axis_rotation((int)k.c[0], k.c[3] != 0.0 ? k.c[1] : (double)u[1] * (k.c[2] - k.c[1]) + k.c[1], a);
      break;
    case SE3_AUG_ROT_3D:
      if (k.c[0] >= 0.0) {
        aug_axis_rotation((int)k.c[0], ((double)u[1] * 2.0) * kPi, a);
      } else {
        const double ra = sqrt(-2.0 * log(1.0 - (double)u[1])), rb = sqrt(-2.0 * log(1.0 - (double)u[3]));
        const double pa = (2.0 * kPi) * (double)u[2], pb = (2.0 * kPi) * (double)u[4];
        double g[4] = {ra * cos(pa), ra * sin(pa), rb * cos(pb), rb * sin(pb)};
        double nrm = sqrt(((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + g[3] * g[3]);
        if (g[0] < 0.0) nrm = -nrm;
        const double r = g[0] / nrm, i = g[1] / nrm, j = g[2] / nrm, q = g[3] / nrm;
        const double two_s = 2.0 / (((r * r + i * i) + j * j) + q * q);
        a[0] = (float)(1.0 - two_s * (j * j + q * q)), a[1] = (float)(two_s * (i * j - q * r)), a[2] = (float)(two_s * (i * q + j * r));
        a[3] = (float)(two_s * (i * j + q * r)), a[4] = (float)(1.0 - two_s * (i * i + q * q)), a[5] = (float)(two_s * (j * q - i * r));
        a[6] = (float)(two_s * (i * q - j * r)), a[7] = (float)(two_s * (j * q + i * r)), a[8] = (float)(1.0 - two_s * (i * i + j * j));
      }
      break;
    case SE3_AUG_CENTER:
#pragma unroll
      for (int j = 0; j < 3; ++j) s[j] = k.c[j] != 0.0 ? -st[6 + j] : 0.f;
      break;
    case SE3_AUG_LINEAR:
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int d = k.c[4] != 0.0 ? 0 : j;
        const bool fixed = k.c[5] != 0.0;
        a[4 * j] = fixed ? (float)k.c[6 + j] : (u[1 + d] * (float)k.c[0]) + (float)k.c[1];
        s[j] = fixed ? (float)k.c[9 + j] : (u[4 + d] * (float)k.c[2]) + (float)k.c[3];
      }
      break;
    case SE3_AUG_MIRROR:
#pragma unroll
      for (int j = 0; j < 3; ++j) a[4 * j] = (k.c[1 + j] != 0.0 && u[1 + j] > (float)k.c[0]) ? -1.f : 1.f;
      break;
    case SE3_AUG_TRANSLATION:
#pragma unroll
      for (int j = 0; j < 3; ++j) s[j] = ((st[3 + j] - st[j]) / 2.f) * (((u[1 + j] * 2.f) - 1.f) * (float)k.c[j]);
      break;
    default: {  // SE3_AUG_STDNORM
      if (counts[b] <= 0) return;  // an empty element keeps its table
      const float f = (float)k.c[0] / fmaxf(fmaxf(st[9], st[10]), st[11]);
      a[0] = a[4] = a[8] = f;
    }
  }
  float* m = affine + (int64_t)b * 12;
  float o[12];
#pragma unroll
  for (int i = 0; i < 4; ++i)  // row 3 of the table is t
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = ((m[3 * i] * a[j]) + (m[3 * i + 1] * a[3 + j])) + (m[3 * i + 2] * a[6 + j]);
      o[3 * i + j] = i == 3 ? v + s[j] : v;
    }
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = o[i];
}

// ----------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(256) void aug_apply_kernel(const float* x, const int32_t* __restrict__ batch_ids,
                                                        int64_t n_rows, const int32_t* __restrict__ n_valid, int32_t n_batches,
                                                        const float* __restrict__ affine, int32_t linear_only,
                                                        const float* __restrict__ noise_draws, float noise_prob, float noise_sigma,
                                                        float noise_clip, float noise_scale, uint32_t seed,
                                                        const uint32_t* __restrict__ seed_device,
                                                        uint32_t step, const uint8_t* __restrict__ ones_mask, float* y) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  float o[3] = {0.f, 0.f, 0.f};
  if (r < present_rows(n_valid, n_rows)) {
    if (ones_mask && ones_mask[r] == 0) {
      o[0] = o[1] = o[2] = 1.f;
    } else {
      const int b = batch_ids[r];
      const bool in_elem = b >= 0 && b < n_batches;
      const float v[3] = {x[r * 3], x[r * 3 + 1], x[r * 3 + 2]};
      aug_transform(affine && in_elem ? affine + (int64_t)b * 12 : nullptr, !linear_only, v, o);
      if (noise_draws && in_elem && noise_draws[(int64_t)b * kDraws] <= noise_prob) {
        const uint32_t key = aug_row_key(aug_seed(seed, seed_device), step, (uint32_t)r);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float u1 = aug_uniform(aug_word(key, 2 * c)), u2 = aug_uniform(aug_word(key, 2 * c + 1));
          float e = (sqrtf(-2.f * logf(1.f - u1)) * cosf(6.283185307179586f * u2)) * noise_sigma;
          if (noise_clip >= 0.f) e = fminf(fmaxf(e, -noise_clip), noise_clip);
          o[c] = o[c] + (e * noise_scale);
        }
      }
    }
  }
  y[r * 3] = o[0], y[r * 3 + 1] = o[1], y[r * 3 + 2] = o[2];
}

// ----------------------------------------------------------------------------------------------------------------- masks
__global__ __launch_bounds__(256) void aug_mask_rows_kernel(int32_t kind, AugConsts k, float prob, const float* __restrict__ pts,
                                                            const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                            const int32_t* __restrict__ n_valid, int32_t n_batches,
                                                            const float* __restrict__ draws, const float* __restrict__ stats,
                                                            uint32_t seed, const uint32_t* __restrict__ seed_device, uint32_t step,
                                                            uint8_t* __restrict__ mask) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  uint8_t keep = 0;
  if (r < present_rows(n_valid, n_rows)) {
    keep = 1;
    const int b = batch_ids[r];
    if (kind != SE3_AUG_CROP_PTS && b >= 0 && b < n_batches && draws[(int64_t)b * kDraws] <= prob) {
      const float* u = draws + (int64_t)b * kDraws;
      if (kind == SE3_AUG_DROP) {
        keep = aug_uniform(aug_word(aug_row_key(aug_seed(seed, seed_device), step, (uint32_t)r), (uint32_t)k.c[1])) > (float)k.c[0];
      } else {  // SE3_AUG_CROP_BOX
        const float* st = stats + (int64_t)b * 12;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float size = fminf((u[1 + j] * (float)k.c[0]) + (float)k.c[1], st[3 + j] - st[j]);
          const float lo = (u[4 + j] * ((st[3 + j] - size) - st[j])) + st[j];
          const float v = pts[r * 3 + j];
          keep &= (v >= lo) & (v <= lo + size);
        }
      }
    }
  }
  mask[r] = keep;
}

__global__ __launch_bounds__(kSelThreads) void aug_crop_pts_kernel(AugConsts k, float prob, const float* __restrict__ pts,
                                                                   const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                                   const int32_t* __restrict__ n_valid, const float* __restrict__ draws,
                                                                   uint8_t* __restrict__ mask) {
  __shared__ int hist[256];
  __shared__ uint32_t sel[2];  // the prefix of the threshold's bits found so far; the rank that is left inside it
  __shared__ int wave_ties[kSelThreads / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* u = draws + (int64_t)b * kDraws;
  if (!(u[0] <= prob)) return;
  const int n = (int)present_rows(n_valid, n_rows);
  const int start = aug_lower_bound(batch_ids, n, b), n_b = aug_lower_bound(batch_ids, n, b + 1) - start;
  const int cap = k.c[0] > 0.0 ? (int)fmin(k.c[0], 2147483647.0) : n_b;
  const int m = min(cap, (int)((double)n_b * k.c[1]));
  if (n_b <= m) return;  // everything kept (the row kernel wrote the ones)
  const int anchor = start + min(max((int)floorf(u[1] * (float)n_b), 0), n_b - 1);
  const float ax = pts[(int64_t)anchor * 3], ay = pts[(int64_t)anchor * 3 + 1], az = pts[(int64_t)anchor * 3 + 2];
  auto dist_bits = [&](int i) {
    const float* p = pts + (int64_t)(start + i) * 3;
    const float dx = p[0] - ax, dy = p[1] - ay, dz = p[2] - az;
    return __float_as_uint(((dx * dx) + (dy * dy)) + (dz * dz));
  };
  if (m <= 0) {
    for (int i = t; i < n_b; i += kSelThreads) mask[start + i] = 0;
    return;
  }
  if (t == 0) sel[0] = 0u, sel[1] = (uint32_t)m;
  for (int pass = 3; pass >= 0; --pass) {
    const int shift = pass * 8;
    const uint32_t above = pass == 3 ? 0u : 0xFFFFFFFFu << (shift + 8);
    if (t < 256) hist[t] = 0;
    __syncthreads();
    const uint32_t prefix = sel[0];
    for (int i = t; i < n_b; i += kSelThreads) {
      const uint32_t d = dist_bits(i);
      if ((d & above) == prefix) atomicAdd(&hist[(d >> shift) & 255u], 1);
    }
    __syncthreads();
    if (t == 0) {
      uint32_t rank = sel[1];  // 1-based among the rows that share the prefix
      int bin = 0;
      while (bin < 255 && (uint32_t)hist[bin] < rank) rank -= (uint32_t)hist[bin++];
      sel[0] = prefix | ((uint32_t)bin << shift), sel[1] = rank;
    }
    __syncthreads();
  }
  const uint32_t thr = sel[0];
  const int ties_wanted = (int)sel[1];  // rows AT the threshold that are kept: the first ones in row order
  int ties_before = 0;                  // (uniform)
  for (int base = 0; base < n_b; base += kSelThreads) {
    const int i = base + t;
    const uint32_t d = i < n_b ? dist_bits(i) : 0xFFFFFFFFu;
    const bool tie = i < n_b && d == thr;
    const uint64_t votes = __ballot(tie);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) wave_ties[wave] = __popcll(votes);
    __syncthreads();
    int before = ties_before, total = 0;
    for (int w = 0; w < kSelThreads / 64; ++w) {
      before += w < wave ? wave_ties[w] : 0;
      total += wave_ties[w];
    }
    before += __popcll(votes & ((1ull << lane) - 1ull));
    if (i < n_b) mask[start + i] = d < thr || (tie && before < ties_wanted);
    ties_before += total;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ compaction
__global__ __launch_bounds__(256) void aug_flags_kernel(const uint8_t* __restrict__ mask, int64_t n_rows,
                                                        const int32_t* __restrict__ n_valid, int32_t* __restrict__ flags) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n_rows) flags[r] = r < present_rows(n_valid, n_rows) && mask[r] != 0;
}

__global__ __launch_bounds__(256) void aug_compact_kernel(const int32_t* __restrict__ flags, const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                          const int32_t* __restrict__ n_valid, int32_t n_batches,
                                                          const int32_t* __restrict__ idx_in, int32_t* __restrict__ idx,
                                                          int32_t* __restrict__ idx_orig, int32_t* __restrict__ n_out, int32_t* __restrict__ counts_out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int total = n_rows > 0 ? pos[n_rows - 1] + flags[n_rows - 1] : 0;
  if (r < n_rows) {
    if (flags[r]) {  // (positions below `total`)
      idx[pos[r]] = (int32_t)r;
      if (idx_orig) idx_orig[pos[r]] = idx_in ? idx_in[r] : (int32_t)r;
    }
    if (r >= total) {
      idx[r] = -1;
      if (idx_orig) idx_orig[r] = -1;
    }
  }
  if (r < n_batches) {
    const int n = (int)present_rows(n_valid, n_rows);
    const int s = aug_lower_bound(batch_ids, n, (int)r), e = aug_lower_bound(batch_ids, n, (int)r + 1);
    counts_out[r] = (e < n_rows ? pos[e] : total) - (s < n_rows ? pos[s] : total);
  }
  if (r == 0) n_out[0] = total;
}

inline int aug_rows_ok(int64_t n_rows, int32_t n_batches) {
  if (n_rows < 0 || n_batches < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows >= (int64_t)1 << 31) return SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}
inline AugConsts aug_consts(const double* consts) {
  AugConsts k;
  for (int i = 0; i < SE3_AUG_CONSTS; ++i) k.c[i] = consts[i];
  return k;
}
inline unsigned row_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

size_t compact_temp_bytes(int64_t n_rows) {
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n_rows);
  return t;
}

}  // namespace

}  // namespace se3

using namespace se3;

extern "C" size_t se3_aug_stats_workspace_bytes(int64_t n_rows, int32_t n_batches) {
  if (aug_rows_ok(n_rows, n_batches) != SE3_OK) return 0;
  return stats_layout(n_rows, n_batches).total;
}

extern "C" int se3_aug_stats(const float* pts, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid,
                             int32_t n_batches, const float* affine, int32_t* counts, float* stats, void* workspace,
                             size_t workspace_bytes, void* stream_) {
  if (int rc = aug_rows_ok(n_rows, n_batches)) return rc;
  if (!counts || !stats || !workspace || (n_rows > 0 && (!pts || !batch_ids))) return SE3_ERR_INVALID_ARGUMENT;
  const StatsLayout l = stats_layout(n_rows, n_batches);
  if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  int32_t *elem_starts = (int32_t*)(ws + l.elem_starts), *slot_starts = (int32_t*)(ws + l.slot_starts);
  double* sums = (double*)(ws + l.sums);
  float* bounds = (float*)(ws + l.bounds);
  ProfScope prof("aug_stats", stream);
  hipLaunchKernelGGL(aug_elements_kernel, dim3(1), dim3(256), 0, stream, batch_ids, n_rows, n_valid, n_batches, elem_starts, slot_starts);
  hipLaunchKernelGGL(aug_stats_chunk_kernel, dim3((unsigned)l.slots), dim3(kChunk), 0, stream, pts, affine, n_batches, elem_starts,
                     slot_starts, sums, bounds);
  hipLaunchKernelGGL(aug_stats_finish_kernel, dim3((unsigned)n_batches), dim3(64), 0, stream, n_batches, elem_starts, slot_starts, sums,
                     bounds, counts, stats);
  return check_launch();
}

extern "C" int se3_aug_affine_step(int32_t kind, const double* consts, float prob, const float* draws, const int32_t* counts,
                                   const float* stats, int32_t n_batches, float* affine, void* stream_) {
  if (n_batches < 1 || !consts || !draws || !affine || kind < SE3_AUG_ROT_AXIS || kind > SE3_AUG_STDNORM) return SE3_ERR_INVALID_ARGUMENT;
  const bool needs_stats = kind == SE3_AUG_CENTER || kind == SE3_AUG_TRANSLATION || kind == SE3_AUG_STDNORM;
  if (needs_stats && (!counts || !stats)) return SE3_ERR_INVALID_ARGUMENT;
  if ((kind == SE3_AUG_ROT_AXIS || (kind == SE3_AUG_ROT_3D && consts[0] >= 0.0)) && !(consts[0] >= 0.0 && consts[0] <= 2.0))
    return SE3_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope prof("aug_affine_step", stream);
  hipLaunchKernelGGL(aug_affine_step_kernel, dim3((unsigned)((n_batches + 63) / 64)), dim3(64), 0, stream, kind, aug_consts(consts), prob,
                     draws, counts, stats, n_batches, affine);
  return check_launch();
}

extern "C" int se3_aug_apply(const float* x, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid, int32_t n_batches,
                             const float* affine, int32_t linear_only, const float* noise_draws, float noise_prob,
                             float noise_sigma, float noise_clip, float noise_scale, uint32_t seed, const uint32_t* seed_device,
                             uint32_t step,
                             const uint8_t* ones_mask, float* y, void* stream_) {
  if (int rc = aug_rows_ok(n_rows, n_batches)) return rc;
  if (n_rows > 0 && (!x || !batch_ids || !y)) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return SE3_OK;
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope prof("aug_apply", stream);
  hipLaunchKernelGGL(aug_apply_kernel, dim3(row_blocks(n_rows)), dim3(256), 0, stream, x, batch_ids, n_rows, n_valid, n_batches, affine,
                     linear_only, noise_draws, noise_prob, noise_sigma, noise_clip, noise_scale, seed, seed_device, step, ones_mask, y);
  return check_launch();
}

extern "C" int se3_aug_keep_mask(int32_t kind, const double* consts, float prob, const float* pts, const int32_t* batch_ids,
                                 int64_t n_rows, const int32_t* n_valid, int32_t n_batches, const float* draws, const float* stats,
                                 uint32_t seed, const uint32_t* seed_device, uint32_t step, uint8_t* mask, void* stream_) {
  if (int rc = aug_rows_ok(n_rows, n_batches)) return rc;
  if (kind < SE3_AUG_DROP || kind > SE3_AUG_CROP_PTS || !consts || !draws) return SE3_ERR_INVALID_ARGUMENT;
  if (kind == SE3_AUG_CROP_BOX && !stats) return SE3_ERR_INVALID_ARGUMENT;
  if (kind == SE3_AUG_DROP && !(consts[1] >= 0.0 && consts[1] <= 5.0)) return SE3_ERR_INVALID_ARGUMENT;  // the words NoiseAug reads
  if (n_rows > 0 && (!pts || !batch_ids || !mask)) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return SE3_OK;
  hipStream_t stream = (hipStream_t)stream_;
  ProfScope prof("aug_keep_mask", stream);
  const AugConsts k = aug_consts(consts);
  hipLaunchKernelGGL(aug_mask_rows_kernel, dim3(row_blocks(n_rows)), dim3(256), 0, stream, kind, k, prob, pts, batch_ids, n_rows, n_valid,
                     n_batches, draws, stats, seed, seed_device, step, mask);
  if (kind == SE3_AUG_CROP_PTS)
    hipLaunchKernelGGL(aug_crop_pts_kernel, dim3((unsigned)n_batches), dim3(kSelThreads), 0, stream, k, prob, pts, batch_ids, n_rows,
                       n_valid, draws, mask);
  return check_launch();
}

extern "C" size_t se3_aug_compact_workspace_bytes(int64_t n_rows) {
  if (aug_rows_ok(n_rows, 1) != SE3_OK) return 0;
  const size_t rows = align_up(sizeof(int32_t) * (size_t)(n_rows > 0 ? n_rows : 1), 256);
  return 2 * rows + align_up(compact_temp_bytes(n_rows), 256);
}

extern "C" int se3_aug_compact(const uint8_t* mask, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid,
                               int32_t n_batches, const int32_t* idx_in, int32_t* idx, int32_t* idx_orig, int32_t* n_out,
                               int32_t* counts_out, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = aug_rows_ok(n_rows, n_batches)) return rc;
  if (!n_out || !counts_out || !workspace || (n_rows > 0 && (!mask || !batch_ids || !idx))) return SE3_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < se3_aug_compact_workspace_bytes(n_rows)) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t rows = align_up(sizeof(int32_t) * (size_t)(n_rows > 0 ? n_rows : 1), 256);
  int32_t *flags = (int32_t*)workspace, *pos = (int32_t*)((char*)workspace + rows);
  ProfScope prof("aug_compact", stream);
  if (n_rows > 0) {
    hipLaunchKernelGGL(aug_flags_kernel, dim3(row_blocks(n_rows)), dim3(256), 0, stream, mask, n_rows, n_valid, flags);
    size_t temp_bytes = compact_temp_bytes(n_rows);
    if (hipcub::DeviceScan::ExclusiveSum((char*)workspace + 2 * rows, temp_bytes, flags, pos, (int)n_rows, stream) != hipSuccess)
      return SE3_ERR_LAUNCH;
  }
  const int64_t threads = n_rows > n_batches ? n_rows : n_batches;
  hipLaunchKernelGGL(aug_compact_kernel, dim3(row_blocks(threads)), dim3(256), 0, stream, flags, pos, batch_ids, n_rows, n_valid, n_batches,
                     idx_in, idx, idx_orig, n_out, counts_out);
  return check_launch();
}
