// Global pooling (include/se3conv_global_pool.h): the feature rows of a cloud -> one row per batch element, in an order of
// additions that the header fixes, and the way back.
//
//   chunks   one thread per (chunk, channel), channels fastest: it walks the present rows of its chunk in ascending order and
//            keeps the partial result of ONE element in registers -- the element of the row it looked at last.  When the id
//            changes it stores that partial into the workspace table `[chunk, element, channel]`, which it has zeroed itself,
//            and takes up the new element's.  A thread owns its column of the table, so nothing is shared and nothing is
//            atomic; sorted ids (the library's own levels) change the element a few times per chunk, shuffled ids at every
//            point, which costs time and never a bit.
//   finish   one thread per (element, channel): the partials of the live chunks in ascending order, the division of avg,
//            `counts`.  The table is dense in (chunk, element) and sorted ids fill a few chunks per element: the row counts
//            say which slots hold something, and only those are read.
//   unpool   one thread per output value.
//
// The row-count word sizes nothing on the host: the grid of `chunks` covers `n_rows`, threads of chunks behind the last
// present point leave at once, and `finish` adds the live chunks only -- the others would add +0.0, an exact identity.
#include "common.h"
#include "../../include/se3conv_global_pool.h"

namespace se3 {
namespace {

enum { kPoolAvg = 0, kPoolMax = 1, kPoolMin = 2, kPoolSum = 3 };
constexpr int64_t kChunk = SE3_GLOBAL_POOL_CHUNK;
static_assert(kChunk > 0 && (kChunk & (kChunk - 1)) == 0, "SE3_GLOBAL_POOL_CHUNK is a power of two");
constexpr int kRowsAhead = 8;  // rows whose loads are issued before the first of them is added: the chain of additions is serial

// one 8-byte slot of the partial table: the fp64 sum, or the extremum and the row that supplied it (-1: none yet)
union Slot {
  double sum;
  struct {
    float best;
    int32_t row;
  } ext;
};
static_assert(sizeof(Slot) == 8, "one slot is 8 bytes");

struct GlobalPoolLayout {
  size_t slots, rows, total;
};

int64_t chunks_of(int64_t n_rows) { return (n_rows + kChunk - 1) / kChunk; }

GlobalPoolLayout global_pool_layout(int64_t n_rows, int32_t n_batches, int32_t channels) {
  const size_t s = (size_t)(n_rows > 0 ? chunks_of(n_rows) : 1);
  GlobalPoolLayout l{};
  l.slots = 0;
  l.rows = align_up(s * (size_t)n_batches * (size_t)channels * sizeof(Slot), 256);
  l.total = l.rows + align_up(s * (size_t)n_batches * sizeof(int32_t), 256);
  return l;
}

template <bool EXTREMUM, bool IS_MAX>
__global__ __launch_bounds__(256) void global_pool_chunks_kernel(const float* __restrict__ x,
                                                                 const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                                 int frames, const int32_t* __restrict__ n_valid, int nb,
                                                                 int c, Slot* slots, int32_t* rows_of) {
  const int64_t present = present_rows(n_valid, n_rows);
  const int64_t live = (present + kChunk - 1) / kChunk;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= live * c) return;
  const int64_t s = t / c;
  const int ch = (int)(t - s * c);
  const bool counts_rows = ch == 0;  // one thread per chunk keeps the row counts of the chunk's elements
  Slot* col = slots + (size_t)s * nb * c + ch;  // this thread's column: col[b * c]
  int32_t* cnt = rows_of + (size_t)s * nb;
  for (int b = 0; b < nb; ++b) {
    Slot z;
    if (EXTREMUM) z.ext.best = 0.f, z.ext.row = -1;
    else z.sum = 0.0;
    col[(size_t)b * c] = z;
    if (counts_rows) cnt[b] = 0;
  }
  const int64_t p0 = s * kChunk, p1 = min(p0 + kChunk, present);
  const int64_t r1 = p1 * frames;
  int64_t p = p0;
  int f = 0;
  int cur = -1, n_cur = 0;  // the element held in registers (-1: none), the rows of it this thread has seen
  Slot acc;
  acc.sum = 0.0;
  for (int64_t r = p0 * frames; r < r1; r += kRowsAhead) {
    float v[kRowsAhead];
    int b[kRowsAhead];
#pragma unroll
    for (int j = 0; j < kRowsAhead; ++j) {
      const bool ok = r + j < r1;  // (neither an absent row nor an absent id is read)
      v[j] = ok ? x[(r + j) * c + ch] : 0.f;
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
      }
      ++n_cur;
      if (EXTREMUM) {
        if (acc.ext.row < 0 || (IS_MAX ? v[j] > acc.ext.best : v[j] < acc.ext.best))
          acc.ext.best = v[j], acc.ext.row = (int32_t)(r + j);
      } else {
        acc.sum += (double)v[j];
      }
    }
  }
  if (cur >= 0) {
    col[(size_t)cur * c] = acc;
    if (counts_rows) cnt[cur] = n_cur;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void global_pool_finish_kernel(const Slot* __restrict__ slots,
                                                                 const int32_t* __restrict__ rows_of, int64_t n_rows,
                                                                 int frames, const int32_t* __restrict__ n_valid, int nb,
                                                                 int c, float* __restrict__ out, int32_t* __restrict__ arg,
                                                                 int32_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nb * c) return;
  const int b = (int)(t / c);
  const int ch = (int)(t - (int64_t)b * c);
  const int64_t live = (present_rows(n_valid, n_rows) + kChunk - 1) / kChunk;
  const size_t step = (size_t)nb * c;
  const Slot* slot = slots + (size_t)b * c + ch;
  // A chunk without a row of the element holds +0.0 (row -1): an exact identity, so its slot is not read.  With sorted ids
  // that is all but a few chunks per element; the row counts that say so are loaded kRowsAhead at a time.
  constexpr bool kExtremum = MODE == kPoolMax || MODE == kPoolMin;
  int64_t rows = 0;
  double total = 0.0;
  float best = 0.f;
  int32_t row = -1;
  for (int64_t s0 = 0; s0 < live; s0 += kRowsAhead) {
    int n[kRowsAhead];
#pragma unroll
    for (int j = 0; j < kRowsAhead; ++j) n[j] = s0 + j < live ? rows_of[(s0 + j) * nb + b] : 0;
#pragma unroll
    for (int j = 0; j < kRowsAhead; ++j) {
      if (n[j] == 0) continue;
      rows += n[j];
      const Slot e = slot[(s0 + j) * step];
      if (kExtremum) {
        if (row < 0 || (MODE == kPoolMax ? e.ext.best > best : e.ext.best < best)) best = e.ext.best, row = e.ext.row;
      } else {
        total += e.sum;
      }
    }
  }
  const int64_t count = rows / frames;
  if (ch == 0) counts[b] = (int32_t)count;
  if (kExtremum) {
    out[t] = best;
    arg[t] = row;
  } else {
    if (MODE == kPoolAvg) out[t] = count > 0 ? (float)(total / (double)(count * frames)) : 0.f;
    else out[t] = (float)total;
    if (arg) arg[t] = -1;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void global_unpool_kernel(const float* __restrict__ vals,
                                                            const int32_t* __restrict__ batch_ids,
                                                            const int32_t* __restrict__ arg,
                                                            const int32_t* __restrict__ counts, int64_t n_rows, int frames,
                                                            const int32_t* __restrict__ n_valid, int nb, int c,
                                                            float* __restrict__ out) {
  const int64_t present = present_rows(n_valid, n_rows);
  const int64_t total = n_rows * frames * c;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / c;
    const int ch = (int)(idx - row * c);
    const int64_t p = row / frames;
    float v = 0.f;
    if (p < present) {
      const int b = batch_ids[p];
      if ((unsigned)b < (unsigned)nb) {
        v = vals[(int64_t)b * c + ch];
        if (MODE == kPoolAvg) v = __fdiv_rn(v, (float)(counts[b] * frames));
        if (MODE == kPoolMax || MODE == kPoolMin) v = arg[(int64_t)b * c + ch] == (int32_t)row ? v : 0.f;
      }
    }
    out[idx] = v;
  }
}

// the checks both entry points share; `values` = n_rows * frames * channels
int global_pool_shape(int64_t n_rows, int32_t frames, int32_t n_batches, int32_t channels, int32_t mode) {
  if (n_rows < 0 || frames < 1 || n_batches < 1 || channels < 1 || mode < kPoolAvg || mode > kPoolSum)
    return SE3_ERR_INVALID_ARGUMENT;
  const int64_t lim = 1ll << 31;
  if ((int64_t)n_batches * channels >= lim) return SE3_ERR_UNSUPPORTED;
  // n_rows * frames * channels >= 2^31, without an overflow on the way
  const int64_t per_point = (int64_t)frames * channels;
  if (per_point >= lim || n_rows >= lim / per_point + (lim % per_point != 0)) return n_rows == 0 ? SE3_OK : SE3_ERR_UNSUPPORTED;
  return SE3_OK;
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" size_t se3_global_pool_workspace_bytes(int64_t n_rows, int32_t frames, int32_t n_batches, int32_t channels) {
  if (global_pool_shape(n_rows, frames, n_batches, channels, kPoolSum) != SE3_OK) return 0;
  return global_pool_layout(n_rows, n_batches, channels).total;
}

extern "C" int se3_global_pool(const float* x, const int32_t* batch_ids, int64_t n_rows, int32_t frames,
                               const int32_t* n_valid, int32_t n_batches, int32_t channels, int32_t mode, float* out,
                               int32_t* arg, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = global_pool_shape(n_rows, frames, n_batches, channels, mode)) return rc;
  const bool extremum = mode == kPoolMax || mode == kPoolMin;
  if (!out || !counts || !workspace || (extremum && !arg) || (n_rows > 0 && (!x || !batch_ids)))
    return SE3_ERR_INVALID_ARGUMENT;
  const GlobalPoolLayout l = global_pool_layout(n_rows, n_batches, channels);
  if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  Slot* slots = (Slot*)((char*)workspace + l.slots);
  int32_t* rows_of = (int32_t*)((char*)workspace + l.rows);
  const int nb = n_batches, c = channels;
  if (n_rows > 0) {
    const dim3 grid(blocks_of(chunks_of(n_rows) * c)), block(256);
#define SE3_GPOOL_CHUNKS(E, M) \
  hipLaunchKernelGGL((global_pool_chunks_kernel<E, M>), grid, block, 0, stream, x, batch_ids, n_rows, frames, n_valid, nb, c, slots, rows_of)
    if (mode == kPoolMax) SE3_GPOOL_CHUNKS(true, true);
    else if (mode == kPoolMin) SE3_GPOOL_CHUNKS(true, false);
    else SE3_GPOOL_CHUNKS(false, false);
#undef SE3_GPOOL_CHUNKS
  }
  const dim3 grid(blocks_of((int64_t)nb * c)), block(256);
#define SE3_GPOOL_FINISH(M) \
  hipLaunchKernelGGL(global_pool_finish_kernel<M>, grid, block, 0, stream, slots, rows_of, n_rows, frames, n_valid, nb, c, out, arg, counts)
  if (mode == kPoolAvg) SE3_GPOOL_FINISH(kPoolAvg);
  else if (mode == kPoolMax) SE3_GPOOL_FINISH(kPoolMax);
  else if (mode == kPoolMin) SE3_GPOOL_FINISH(kPoolMin);
  else SE3_GPOOL_FINISH(kPoolSum);
#undef SE3_GPOOL_FINISH
  return check_launch();
}

extern "C" int se3_global_unpool(const float* vals, const int32_t* batch_ids, const int32_t* arg, const int32_t* counts,
                                 int64_t n_rows, int32_t frames, const int32_t* n_valid, int32_t n_batches, int32_t channels,
                                 int32_t mode, float* out, void* stream_) {
  if (int rc = global_pool_shape(n_rows, frames, n_batches, channels, mode)) return rc;
  if (n_rows == 0) return SE3_OK;
  if (!vals || !batch_ids || !out || ((mode == kPoolMax || mode == kPoolMin) && !arg) || (mode == kPoolAvg && !counts))
    return SE3_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t values = n_rows * frames * channels;
  const dim3 grid(blocks_of(values) < 8192u ? blocks_of(values) : 8192u), block(256);
#define SE3_GUNPOOL(M) \
  hipLaunchKernelGGL(global_unpool_kernel<M>, grid, block, 0, stream, vals, batch_ids, arg, counts, n_rows, frames, n_valid, n_batches, channels, out)
  if (mode == kPoolAvg) SE3_GUNPOOL(kPoolAvg);
  else if (mode == kPoolMax) SE3_GUNPOOL(kPoolMax);
  else if (mode == kPoolMin) SE3_GUNPOOL(kPoolMin);
  else SE3_GUNPOOL(kPoolSum);
#undef SE3_GUNPOOL
  return check_launch();
}
