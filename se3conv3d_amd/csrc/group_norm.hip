// Point-cloud group norm (include/se3conv_group_norm.h): statistics per (batch element, channel group) in the chunked fp64
// order of global_pool.hip, the normalisation and its gradient row-wise behind them.  Forward and backward are the same four
// stages, and the first two are the same code:
//
//   chunks   one thread per (chunk, channel), channels fastest: it walks the present rows of its chunk in ascending order and
//            keeps the two partial sums of ONE element in registers -- the element of the row it looked at last (forward: x and
//            x * x; backward: dy and dy * xhat).  When the id changes it stores them into the workspace table
//            `[chunk, element, channel]`, which it has zeroed itself, and takes up the new element's.  A thread owns its column
//            of the table: nothing is shared, nothing is atomic.
//   totals   one wavefront per (element, 64 channels): the partials of the live chunks in ascending order ->
//            `[element, channel]`, and the element's point count.  The row counts per (chunk, element) say which slots hold
//            something; only those are read.
//   finish   forward: one thread per (element, group) -> save_mean, save_invstd.  backward: one thread per (element, group)
//            -> the two row-wise constants a, q, and one per channel -> dgamma, dbeta.
//   rows     one thread per four values of y / dx (one where the channel count is no multiple of four).
//
// The row-count word sizes nothing on the host: the grid of `chunks` covers `n_rows`, threads of chunks behind the last
// present point leave at once, and `totals` adds the live chunks only -- the others would add +0.0, an exact identity.
// Every arithmetic step the header fixes stands in a function under `fp contract(off)`: hipcc would otherwise fuse a product
// into the addition behind it, and the result would no longer be the one numpy gives.
#include "common.h"
#include "../../include/se3conv_group_norm.h"

namespace se3 {
namespace {

constexpr int64_t kChunk = SE3_GROUP_NORM_CHUNK;
static_assert(kChunk > 0 && (kChunk & (kChunk - 1)) == 0, "SE3_GROUP_NORM_CHUNK is a power of two");
constexpr int kRowsAhead = 8;  // rows whose loads are issued before the first of them is added: the chain of additions is serial

struct Pair {
  double a, b;
};
static_assert(sizeof(Pair) == 16, "one slot is 16 bytes");

struct GroupNormLayout {
  size_t slots, rows, totals, counts, consts, total;
};

int64_t chunks_of(int64_t n_rows) { return (n_rows + kChunk - 1) / kChunk; }

GroupNormLayout group_norm_layout(int64_t n_rows, int32_t n_batches, int32_t channels, int32_t groups) {
  const size_t s = (size_t)(n_rows > 0 ? chunks_of(n_rows) : 1);
  GroupNormLayout l{};
  l.slots = 0;
  l.rows = align_up(s * (size_t)n_batches * (size_t)channels * sizeof(Pair), 256);
  l.totals = l.rows + align_up(s * (size_t)n_batches * sizeof(int32_t), 256);
  l.counts = l.totals + align_up((size_t)n_batches * (size_t)channels * sizeof(Pair), 256);
  l.consts = l.counts + align_up((size_t)n_batches * sizeof(int32_t), 256);
  l.total = l.consts + align_up((size_t)n_batches * (size_t)groups * 2 * sizeof(float), 256);
  return l;
}

__device__ __forceinline__ float gn_xhat(float x, float mean, float invstd) {
#pragma clang fp contract(off)
  const float d = x - mean;
  return d * invstd;
}

__device__ __forceinline__ float gn_affine(float xhat, float gamma, float beta) {
#pragma clang fp contract(off)
  const float p = xhat * gamma;
  return p + beta;
}

__device__ __forceinline__ float gn_dx(float dy, float xhat, float gamma, float invstd, float a, float q) {
#pragma clang fp contract(off)
  const float gd = gamma * dy;
  const float t = gd - a;
  const float xq = xhat * q;
  const float u = t - xq;
  return invstd * u;
}

// acc += (double)v * (double)w: the product of two floats is exact in fp64, so fused or not it is the same number
__device__ __forceinline__ double gn_add_product(double acc, float v, float w) {
#pragma clang fp contract(off)
  const double p = (double)v * (double)w;
  return acc + p;
}

__device__ __forceinline__ double gn_add_scaled(double acc, float g, double t) {
#pragma clang fp contract(off)
  const double p = (double)g * t;
  return acc + p;
}

__device__ __forceinline__ void gn_stats(double s1, double s2, double n, float eps, float* mean, float* invstd) {
#pragma clang fp contract(off)
  const double m = s1 / n;
  const double e2 = s2 / n;
  const double mm = m * m;
  double var = e2 - mm;
  var = var > 0.0 ? var : 0.0;
  const double ve = var + (double)eps;
  *mean = (float)m;
  *invstd = (float)(1.0 / sqrt(ve));
}

// BACKWARD: the second sum is dy * xhat (xhat from x and the saved statistics of the row's element); else x * x
template <bool BACKWARD>
__global__ __launch_bounds__(256) void group_norm_chunks_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ save_mean,
                                                                const float* __restrict__ save_invstd,
                                                                const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                                int frames, const int32_t* __restrict__ n_valid, int nb, int c,
                                                                int groups, Pair* slots, int32_t* rows_of) {
  const int64_t present = present_rows(n_valid, n_rows);
  const int64_t live = (present + kChunk - 1) / kChunk;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= live * c) return;
  const int64_t s = t / c;
  const int ch = (int)(t - s * c);
  const int grp = ch % groups;
  const bool counts_rows = ch == 0;  // one thread per chunk keeps the row counts of the chunk's elements
  Pair* col = slots + (size_t)s * nb * c + ch;  // this thread's column: col[b * c]
  int32_t* cnt = rows_of + (size_t)s * nb;
  for (int b = 0; b < nb; ++b) {
    col[(size_t)b * c] = Pair{0.0, 0.0};
    if (counts_rows) cnt[b] = 0;
  }
  const int64_t p0 = s * kChunk, p1 = min(p0 + kChunk, present);
  const int64_t r1 = p1 * frames;
  int64_t p = p0;
  int f = 0;
  int cur = -1, n_cur = 0;  // the element held in registers (-1: none), the rows of it this thread has seen
  Pair acc{0.0, 0.0};
  float mean = 0.f, invstd = 0.f;
  for (int64_t r = p0 * frames; r < r1; r += kRowsAhead) {
    float v[kRowsAhead], g[kRowsAhead];
    int b[kRowsAhead];
#pragma unroll
    for (int j = 0; j < kRowsAhead; ++j) {
      const bool ok = r + j < r1;  // (neither an absent row nor an absent id is read)
      v[j] = ok ? x[(r + j) * c + ch] : 0.f;
      g[j] = BACKWARD && ok ? dy[(r + j) * c + ch] : 0.f;
      b[j] = ok ? batch_ids[p] : -1;
      if (++f == frames) f = 0, ++p;
    }
#pragma unroll
    for (int j = 0; j < kRowsAhead; ++j) {
      if ((unsigned)b[j] >= (unsigned)nb) continue;  // behind the chunk's end, or a point of no element
      if (b[j] != cur) {
        if (cur >= 0) {
          col[(size_t)cur * c] = acc;
          if (counts_rows) cnt[cur] = n_cur;
        }
        cur = b[j];
        acc = col[(size_t)cur * c];
        n_cur = counts_rows ? cnt[cur] : 0;
        if (BACKWARD) mean = save_mean[(size_t)cur * groups + grp], invstd = save_invstd[(size_t)cur * groups + grp];
      }
      ++n_cur;
      if (BACKWARD) {
        acc.a += (double)g[j];
        acc.b = gn_add_product(acc.b, g[j], gn_xhat(v[j], mean, invstd));
      } else {
        acc.a += (double)v[j];
        acc.b = gn_add_product(acc.b, v[j], v[j]);
      }
    }
  }
  if (cur >= 0) {
    col[(size_t)cur * c] = acc;
    if (counts_rows) cnt[cur] = n_cur;
  }
}

constexpr int kScan = 4;    // row counts a lane loads per round of the totals pass: a round covers 64 * kScan chunks
constexpr int kSlotsAhead = 8;  // live slots whose loads are issued before the first of them is added

// One WAVEFRONT per (element, 64 channels), lanes = channels.  Which chunks hold rows of the element is found by the whole
// wavefront -- each lane looks at the row counts of other chunks, a ballot turns them into a mask -- and the walk over the set
// bits is wave-uniform: the live slots are loaded kSlotsAhead at a time (64 lanes, 1 KiB per slot row) and added in ascending
// chunk order.  A slot that is not loaded counts as +0.0, the exact identity it would hold.
__global__ __launch_bounds__(256) void group_norm_totals_kernel(const Pair* __restrict__ slots,
                                                                const int32_t* __restrict__ rows_of, int64_t n_rows, int frames,
                                                                const int32_t* __restrict__ n_valid, int nb, int c,
                                                                Pair* __restrict__ totals, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int cblocks = (c + 63) / 64;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= (int64_t)nb * cblocks) return;  // (the whole wavefront)
  const int b = (int)(unit / cblocks);
  const int cb = (int)(unit - (int64_t)b * cblocks);
  const int ch = cb * 64 + lane;
  const bool has = ch < c;
  const int64_t live = (present_rows(n_valid, n_rows) + kChunk - 1) / kChunk;
  const size_t step = (size_t)nb * c;
  const Pair* slot = slots + (size_t)b * c + (has ? ch : 0);
  int rows = 0;  // of the chunks this lane looked at
  Pair total{0.0, 0.0};
  for (int64_t s0 = 0; s0 < live; s0 += 64 * kScan) {
    int n[kScan];
#pragma unroll
    for (int k = 0; k < kScan; ++k) {
      const int64_t s = s0 + k * 64 + lane;
      n[k] = s < live ? rows_of[s * nb + b] : 0;
      rows += n[k];
    }
#pragma unroll
    for (int k = 0; k < kScan; ++k) {
      unsigned long long mask = __ballot(n[k] != 0);
      const int64_t base = s0 + k * 64;
      while (mask) {
        Pair e[kSlotsAhead];
#pragma unroll
        for (int j = 0; j < kSlotsAhead; ++j) {
          e[j] = Pair{0.0, 0.0};
          if (mask) {
            const int bit = __builtin_ctzll(mask);
            mask &= mask - 1;
            if (has) e[j] = slot[(size_t)(base + bit) * step];
          }
        }
#pragma unroll
        for (int j = 0; j < kSlotsAhead; ++j) {
          total.a += e[j].a;
          total.b += e[j].b;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) rows += __shfl_xor(rows, off);
  if (has) totals[(size_t)b * c + ch] = total;
  if (cb == 0 && lane == 0) counts[b] = rows / frames;
}

__global__ __launch_bounds__(256) void group_norm_stats_kernel(const Pair* __restrict__ totals,
                                                               const int32_t* __restrict__ counts, int frames, int nb, int c,
                                                               int groups, float eps, float* __restrict__ save_mean,
                                                               float* __restrict__ save_invstd) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nb * groups) return;
  const int b = t / groups, j = t - b * groups;
  const int64_t points = counts[b];
  float mean = 0.f, invstd = 0.f;
  if (points > 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int ch = j; ch < c; ch += groups) {
      const Pair e = totals[(size_t)b * c + ch];
      s1 += e.a;
      s2 += e.b;
    }
    gn_stats(s1, s2, (double)(points * frames * (c / groups)), eps, &mean, &invstd);
  }
  save_mean[t] = mean;
  save_invstd[t] = invstd;
}

// threads [0, nb * groups): a, q of an (element, group); threads [nb * groups, nb * groups + c): dgamma, dbeta of a channel
__global__ __launch_bounds__(256) void group_norm_grads_kernel(const Pair* __restrict__ totals,
                                                               const int32_t* __restrict__ counts,
                                                               const float* __restrict__ gamma, int frames, int nb, int c,
                                                               int groups, float* __restrict__ consts,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < (int64_t)nb * groups) {
    const int b = (int)(t / groups), j = (int)(t - (int64_t)b * groups);
    const int64_t points = counts[b];
    float a = 0.f, q = 0.f;
    if (points > 0) {
      double sa = 0.0, sq = 0.0;
      for (int ch = j; ch < c; ch += groups) {
        const Pair e = totals[(size_t)b * c + ch];
        const float ga = gamma[ch];
        sa = gn_add_scaled(sa, ga, e.a);
        sq = gn_add_scaled(sq, ga, e.b);
      }
      const double n = (double)(points * frames * (c / groups));
      a = (float)(sa / n);
      q = (float)(sq / n);
    }
    consts[2 * t] = a;
    consts[2 * t + 1] = q;
    return;
  }
  if (t - (int64_t)nb * groups >= c) return;
  const int ch = (int)(t - (int64_t)nb * groups);
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < nb; ++b) {
    const Pair e = totals[(size_t)b * c + ch];
    s1 += e.a;
    s2 += e.b;
  }
  dbeta[ch] = (float)s1;
  dgamma[ch] = (float)s2;
}

// One thread per VEC adjacent channels of a row (VEC = 4 where the channel count allows).  The host has refused
// n_rows * frames * channels >= 2^31, so the index arithmetic is 32-bit.
template <bool BACKWARD, int VEC>
__global__ __launch_bounds__(256) void group_norm_rows_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ save_mean,
                                                              const float* __restrict__ save_invstd,
                                                              const float* __restrict__ consts,
                                                              const int32_t* __restrict__ batch_ids, int64_t n_rows, int frames,
                                                              const int32_t* __restrict__ n_valid, int nb, int c, int groups,
                                                              float* __restrict__ out) {
  const uint32_t present = (uint32_t)present_rows(n_valid, n_rows);
  const uint32_t cv = (uint32_t)c / VEC;
  const uint32_t total = (uint32_t)(n_rows * frames) * cv;
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const uint32_t row = idx / cv;
    const uint32_t ch = (idx - row * cv) * VEC;
    const uint32_t p = row / (uint32_t)frames;
    const size_t at = (size_t)row * c + ch;
    float v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    const int b = p < present ? batch_ids[p] : -1;  // (an absent id is not read)
    if ((unsigned)b < (unsigned)nb) {
      float xv[VEC], gv[VEC];
      if (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(x + at);
        xv[0] = t.x, xv[1] = t.y, xv[2] = t.z, xv[3] = t.w;
        if (BACKWARD) {
          const float4 u = *reinterpret_cast<const float4*>(dy + at);
          gv[0] = u.x, gv[1] = u.y, gv[2] = u.z, gv[3] = u.w;
        }
      } else {
        xv[0] = x[at];
        if (BACKWARD) gv[0] = dy[at];
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const int slot = b * groups + (int)((ch + i) % (uint32_t)groups);
        const float r = save_invstd[slot];
        const float xhat = gn_xhat(xv[i], save_mean[slot], r);
        if (BACKWARD) v[i] = gn_dx(gv[i], xhat, gamma[ch + i], r, consts[2 * slot], consts[2 * slot + 1]);
        else v[i] = gn_affine(xhat, gamma[ch + i], beta[ch + i]);
      }
    }
    if (VEC == 4) *reinterpret_cast<float4*>(out + at) = make_float4(v[0], v[1], v[2], v[3]);
    else out[at] = v[0];
  }
}

// the checks both entry points share
int group_norm_shape(int64_t n_rows, int32_t frames, int32_t n_batches, int32_t channels, int32_t groups) {
  if (n_rows < 0 || frames < 1 || n_batches < 1 || channels < 1 || groups < 1 || channels % groups != 0)
    return SE3_ERR_INVALID_ARGUMENT;
  const int64_t lim = 1ll << 31;
  if ((int64_t)n_batches * channels >= lim) return SE3_ERR_UNSUPPORTED;
  // n_rows * frames * channels >= 2^31, without an overflow on the way
  const int64_t per_point = (int64_t)frames * channels;
  if (per_point >= lim || n_rows >= lim / per_point + (lim % per_point != 0)) return n_rows == 0 ? SE3_OK : SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + 255) / 256); }

struct GroupNormTables {
  Pair* slots;
  int32_t* rows_of;
  Pair* totals;
  int32_t* counts;
  float* consts;
};

GroupNormTables group_norm_tables(void* workspace, const GroupNormLayout& l) {
  char* w = (char*)workspace;
  return {(Pair*)(w + l.slots), (int32_t*)(w + l.rows), (Pair*)(w + l.totals), (int32_t*)(w + l.counts), (float*)(w + l.consts)};
}

// stages 1 and 2 of either call
template <bool BACKWARD>
void group_norm_sums(const float* x, const float* dy, const float* save_mean, const float* save_invstd, const int32_t* batch_ids,
                     int64_t n_rows, int frames, const int32_t* n_valid, int nb, int c, int groups, const GroupNormTables& t,
                     hipStream_t stream) {
  if (n_rows > 0)
    hipLaunchKernelGGL(group_norm_chunks_kernel<BACKWARD>, dim3(blocks_of(chunks_of(n_rows) * c)), dim3(256), 0, stream, x, dy,
                       save_mean, save_invstd, batch_ids, n_rows, frames, n_valid, nb, c, groups, t.slots, t.rows_of);
  const int64_t waves = (int64_t)nb * ((c + 63) / 64);  // one per (element, 64 channels), four to a block
  hipLaunchKernelGGL(group_norm_totals_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, t.slots, t.rows_of, n_rows,
                     frames, n_valid, nb, c, t.totals, t.counts);
}

// stage 4 of either call
template <bool BACKWARD>
void group_norm_rows(const float* x, const float* dy, const float* gamma, const float* beta, const float* save_mean,
                     const float* save_invstd, const float* consts, const int32_t* batch_ids, int64_t n_rows, int frames,
                     const int32_t* n_valid, int nb, int c, int groups, float* out, hipStream_t stream) {
  // rows of 4n floats behind 16-byte aligned bases: every float4 is aligned (the arithmetic is the same either way)
  const bool vec4 = c % 4 == 0 && ((uintptr_t)x | (uintptr_t)dy | (uintptr_t)out) % 16 == 0;
  const unsigned blocks = blocks_of(n_rows * frames * (vec4 ? c / 4 : c));
  const dim3 grid(blocks < 8192u ? blocks : 8192u), block(256);
  if (vec4)
    hipLaunchKernelGGL((group_norm_rows_kernel<BACKWARD, 4>), grid, block, 0, stream, x, dy, gamma, beta, save_mean, save_invstd,
                       consts, batch_ids, n_rows, frames, n_valid, nb, c, groups, out);
  else
    hipLaunchKernelGGL((group_norm_rows_kernel<BACKWARD, 1>), grid, block, 0, stream, x, dy, gamma, beta, save_mean, save_invstd,
                       consts, batch_ids, n_rows, frames, n_valid, nb, c, groups, out);
}

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" size_t se3_group_norm_workspace_bytes(int64_t n_rows, int32_t frames, int32_t n_batches, int32_t channels,
                                                 int32_t groups) {
  if (group_norm_shape(n_rows, frames, n_batches, channels, groups) != SE3_OK) return 0;
  return group_norm_layout(n_rows, n_batches, channels, groups).total;
}

extern "C" int se3_group_norm_fwd(const float* x, const float* gamma, const float* beta, const int32_t* batch_ids,
                                  int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t n_batches, int32_t channels,
                                  int32_t groups, float eps, float* y, float* save_mean, float* save_invstd, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
  if (int rc = group_norm_shape(n_rows, frames, n_batches, channels, groups)) return rc;
  if (!gamma || !beta || !save_mean || !save_invstd || !workspace || (n_rows > 0 && (!x || !batch_ids || !y)))
    return SE3_ERR_INVALID_ARGUMENT;
  const GroupNormLayout l = group_norm_layout(n_rows, n_batches, channels, groups);
  if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const GroupNormTables t = group_norm_tables(workspace, l);
  const int nb = n_batches, c = channels;
  group_norm_sums<false>(x, nullptr, nullptr, nullptr, batch_ids, n_rows, frames, n_valid, nb, c, groups, t, stream);
  hipLaunchKernelGGL(group_norm_stats_kernel, dim3(blocks_of((int64_t)nb * groups)), dim3(256), 0, stream, t.totals, t.counts,
                     frames, nb, c, groups, eps, save_mean, save_invstd);
  if (n_rows > 0)
    group_norm_rows<false>(x, nullptr, gamma, beta, save_mean, save_invstd, nullptr, batch_ids, n_rows, frames, n_valid, nb, c,
                           groups, y, stream);
  return check_launch();
}

extern "C" int se3_group_norm_bwd(const float* dy, const float* x, const float* gamma, const float* save_mean,
                                  const float* save_invstd, const int32_t* batch_ids, int64_t n_rows, int32_t frames,
                                  const int32_t* n_valid, int32_t n_batches, int32_t channels, int32_t groups, float* dx,
                                  float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = group_norm_shape(n_rows, frames, n_batches, channels, groups)) return rc;
  if (!gamma || !save_mean || !save_invstd || !dgamma || !dbeta || !workspace ||
      (n_rows > 0 && (!dy || !x || !batch_ids || !dx)))
    return SE3_ERR_INVALID_ARGUMENT;
  const GroupNormLayout l = group_norm_layout(n_rows, n_batches, channels, groups);
  if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const GroupNormTables t = group_norm_tables(workspace, l);
  const int nb = n_batches, c = channels;
  group_norm_sums<true>(x, dy, save_mean, save_invstd, batch_ids, n_rows, frames, n_valid, nb, c, groups, t, stream);
  hipLaunchKernelGGL(group_norm_grads_kernel, dim3(blocks_of((int64_t)nb * groups + c)), dim3(256), 0, stream, t.totals,
                     t.counts, gamma, frames, nb, c, groups, t.consts, dgamma, dbeta);
  if (n_rows > 0)
    group_norm_rows<true>(x, dy, gamma, nullptr, save_mean, save_invstd, t.consts, batch_ids, n_rows, frames, n_valid, nb, c,
                          groups, dx, stream);
  return check_launch();
}
