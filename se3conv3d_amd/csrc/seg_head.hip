// Loss and metrics head (include/se3conv_seg_head.h): the mean smoothed cross-entropy over the rows that count, its gradient
// and the per-class counters, in the chunked fp64 order of global_pool.hip.  Three kernels:
//
//   rows     one workgroup of 256 threads per chunk of 256 rows.  It stages the chunk's `256 x classes` floats in LDS with
//            coalesced 16-byte loads (row stride `classes | 1` words, so that the 32 lanes of an LDS access that walk their
//            own rows hit 32 banks), one lane then does one row out of LDS: first maximum, fp64 log-sum-exp, the row's loss.
//            The row losses are staged in LDS and ONE lane adds them in ascending row order; the three histograms of the
//            workgroup are built with integer LDS atomics.  Partial sum, partial count and histograms go to the workspace.
//   finish   block 0: the partials of the live chunks in ascending order -> loss, count; the other blocks: one thread per
//            tally, the live chunks' histogram entries added to it.  `tallies += ...` is the one read-modify-write of the
//            library, by exactly one thread per word.
//   grad     one launch over the same tile: stage, every lane overwrites its row of the tile with the gradient (zeros where
//            the row does not count), and the tile goes out with coalesced stores.
//
// Rows wider than SE3_SEG_HEAD_TILE_CLASSES do not fit the tile: the same kernels, instantiated without the staging, let a lane
// read (and, in `grad`, write) its row in memory.  The launcher picks; both forms run the same row arithmetic in the same
// order and give the same bits.
//
// The row-count word sizes nothing on the host: the grid covers `n_rows`, workgroups behind the last present row write their
// zeros (`lse`, gradient rows) and leave, and `finish` adds the live chunks only.  The row arithmetic stands in functions under
// `fp contract(off)`, so that it is the sequence of roundings the header states.
#include "common.h"
#include "../../include/se3conv_seg_head.h"

namespace se3 {
namespace {

constexpr int kChunk = SE3_SEG_HEAD_CHUNK;
constexpr int kTileClasses = SE3_SEG_HEAD_TILE_CLASSES;
constexpr int kMaxClasses = 1024;
static_assert(kChunk == 256, "one lane of a 256-thread workgroup per row of a chunk");

__host__ __device__ constexpr int tile_stride(int classes) { return classes | 1; }  // words: odd
__host__ __device__ constexpr size_t tile_bytes(int classes) { return (size_t)kChunk * tile_stride(classes) * sizeof(float); }
// the widest tile, the staged row losses and three histograms fit the 64 KiB a workgroup gets without asking for more
static_assert(tile_bytes(kTileClasses) + kChunk * sizeof(double) + 3 * kTileClasses * sizeof(int) <= 64 * 1024, "LDS tile");

struct SegHeadLayout {
  size_t sums, counts, hists, total;
};

int64_t chunks_of(int64_t n_rows) { return (n_rows + kChunk - 1) / kChunk; }

SegHeadLayout seg_head_layout(int64_t n_rows, int32_t classes) {
  const size_t s = (size_t)(n_rows > 0 ? chunks_of(n_rows) : 1);
  SegHeadLayout l{};
  l.sums = 0;
  l.counts = l.sums + align_up(s * sizeof(double), 256);
  l.hists = l.counts + align_up(s * sizeof(int32_t), 256);
  l.total = l.hists + align_up(s * 3 * (size_t)classes * sizeof(int32_t), 256);
  return l;
}

__device__ __forceinline__ int64_t load_label(const void* __restrict__ labels, int label_bits, int64_t r) {
  return label_bits == 64 ? ((const int64_t*)labels)[r] : (int64_t)((const int32_t*)labels)[r];
}

__device__ __forceinline__ bool row_counts(int64_t label, int classes, const uint8_t* __restrict__ counted) {
  return label >= 0 && label < classes && (!counted || counted[label] != 0);
}

// `n` consecutive floats at `src` (whole rows of `classes`) -> the tile, row stride `stride`.  16-byte loads where `vec4`
// says that `src` is aligned; nothing behind `src + n` is read.
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int n, int classes, int stride, float* tile, bool vec4) {
  const int t = threadIdx.x;
  int done = 0;
  if (vec4) {
    const int n4 = n >> 2;
    for (int i = t; i < n4; i += kChunk) {
      const float4 v = reinterpret_cast<const float4*>(src)[i];
      const float w[4] = {v.x, v.y, v.z, v.w};
      int row = (i * 4) / classes, col = i * 4 - row * classes;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        tile[row * stride + col] = w[j];
        if (++col == classes) col = 0, ++row;
      }
    }
    done = n4 << 2;
  }
  for (int e = done + t; e < n; e += kChunk) {
    const int row = e / classes;
    tile[row * stride + (e - row * classes)] = src[e];
  }
}

// the tile -> `n` consecutive floats at `dst`
__device__ __forceinline__ void unstage_rows(const float* tile, float* __restrict__ dst, int n, int classes, int stride, bool vec4) {
  const int t = threadIdx.x;
  int done = 0;
  if (vec4) {
    const int n4 = n >> 2;
    for (int i = t; i < n4; i += kChunk) {
      float w[4];
      int row = (i * 4) / classes, col = i * 4 - row * classes;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = tile[row * stride + col];
        if (++col == classes) col = 0, ++row;
      }
      reinterpret_cast<float4*>(dst)[i] = make_float4(w[0], w[1], w[2], w[3]);
    }
    done = n4 << 2;
  }
  for (int e = done + t; e < n; e += kChunk) {
    const int row = e / classes;
    dst[e] = tile[row * stride + (e - row * classes)];
  }
}

struct RowResult {
  double lse, loss;
  int pred;
};

// one counted row, as the header states it
__device__ __forceinline__ RowResult seg_row(const float* x, int classes, int label, double eps) {
#pragma clang fp contract(off)
  float best = x[0];
  int pred = 0;
  double sx = (double)best;
  for (int c = 1; c < classes; ++c) {
    const float v = x[c];
    sx += (double)v;
    if (v > best) best = v, pred = c;  // the first maximum; a NaN never replaces
  }
  const double m = (double)best;
  double se = 0.0;
  for (int c = 0; c < classes; ++c) se += exp((double)x[c] - m);
  const double lse = m + log(se);
  const double k = (double)classes;
  const double nll = lse - (double)x[label];
  const double kl = k * lse;
  const double smooth = kl - sx;
  const double a = (1.0 - eps) * nll;
  const double b = (eps / k) * smooth;
  return RowResult{lse, a + b, pred};
}

__device__ __forceinline__ float seg_grad(float x, double lse, double q, double g, double cnt) {
#pragma clang fp contract(off)
  const double p = exp((double)x - lse);
  const double d = p - q;
  const double gd = g * d;
  return (float)(gd / cnt);
}

template <bool STAGED>
__global__ __launch_bounds__(256) void seg_loss_rows_kernel(const float* __restrict__ logits, const void* __restrict__ labels,
                                                            int label_bits, const uint8_t* __restrict__ counted, int64_t n_rows,
                                                            const int32_t* __restrict__ n_valid, int classes, float smoothing,
                                                            double* __restrict__ lse_out, bool want_hist, bool vec4,
                                                            double* __restrict__ part_sum, int32_t* __restrict__ part_count,
                                                            int32_t* __restrict__ part_hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int stride = tile_stride(classes);
  float* tile = reinterpret_cast<float*>(smem);
  double* losses = reinterpret_cast<double*>(smem + (STAGED ? tile_bytes(classes) : 0));  // (256 * stride words: 8-byte aligned)
  int* hist = reinterpret_cast<int*>(losses + kChunk);
  const int t = threadIdx.x;
  const int64_t present = present_rows(n_valid, n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * kChunk, r = r0 + t;
  if (r0 >= present) {  // (the whole workgroup) a chunk without a present row: its zeros, and no partial -- `finish` reads none
    if (lse_out && r < n_rows) lse_out[r] = 0.0;
    return;
  }
  const int rows = (int)min((int64_t)kChunk, present - r0);
  if (STAGED) stage_rows(logits + r0 * classes, rows * classes, classes, stride, tile, vec4);
  for (int i = t; i < 3 * classes; i += kChunk) hist[i] = 0;
  __syncthreads();
  bool ok = false;
  RowResult res{0.0, 0.0, 0};
  if (t < rows) {  // (neither an absent row nor an absent label is read)
    const int64_t label = load_label(labels, label_bits, r);
    ok = row_counts(label, classes, counted);
    if (ok) {
      const float* x = STAGED ? tile + t * stride : logits + r * classes;
      res = seg_row(x, classes, (int)label, (double)smoothing);
      if (want_hist) {
        atomicAdd(&hist[label], 1);
        atomicAdd(&hist[classes + res.pred], 1);
        if (res.pred == (int)label) atomicAdd(&hist[2 * classes + label], 1);
      }
    }
  }
  losses[t] = res.loss;  // +0.0 for a row that does not count: an exact identity of the sum below, which is never -0.0
  if (lse_out && r < n_rows) lse_out[r] = res.lse;
  const int n_ok = __syncthreads_count(ok);
  if (t == 0) {
    double acc = 0.0;
    for (int i = 0; i < rows; ++i) acc += losses[i];
    part_sum[blockIdx.x] = acc;
    part_count[blockIdx.x] = n_ok;
  }
  if (want_hist)
    for (int i = t; i < 3 * classes; i += kChunk) part_hist[(size_t)blockIdx.x * 3 * classes + i] = hist[i];
}

// block 0: loss and count; blocks 1 ..: one thread per word of `tallies` (launched only with tallies)
__global__ __launch_bounds__(256) void seg_loss_finish_kernel(const double* __restrict__ part_sum,
                                                              const int32_t* __restrict__ part_count,
                                                              const int32_t* __restrict__ part_hist, int64_t n_rows,
                                                              const int32_t* __restrict__ n_valid, int classes,
                                                              float* __restrict__ loss, int32_t* __restrict__ count,
                                                              int64_t* tallies) {
  const int64_t live = (present_rows(n_valid, n_rows) + kChunk - 1) / kChunk;
  const int t = threadIdx.x;
  if (blockIdx.x > 0) {
    const int i = (blockIdx.x - 1) * 256 + t;
    if (i >= 3 * classes) return;
    int64_t sum = 0;
    for (int64_t s = 0; s < live; ++s) sum += part_hist[(size_t)s * 3 * classes + i];
    tallies[i] += sum;
    return;
  }
  __shared__ double stage[256];
  __shared__ int counted_rows;
  if (t == 0) counted_rows = 0;
  double total = 0.0;  // (thread 0's)
  int mine = 0;
  for (int64_t s0 = 0; s0 < live; s0 += 256) {
    const int64_t s = s0 + t;
    __syncthreads();  // the round before has been added
    stage[t] = s < live ? part_sum[s] : 0.0;
    if (s < live) mine += part_count[s];
    __syncthreads();
    if (t == 0) {
      const int n = (int)min((int64_t)256, live - s0);
      for (int i = 0; i < n; ++i) total += stage[i];
    }
  }
  __syncthreads();
  atomicAdd(&counted_rows, mine);  // (an integer, in LDS)
  __syncthreads();
  if (t == 0) {
    const int n = counted_rows;
    *count = n;
    *loss = (float)(total / (double)max(n, 1));
  }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void seg_loss_grad_kernel(const float* __restrict__ logits, const void* __restrict__ labels,
                                                            int label_bits, const uint8_t* __restrict__ counted,
                                                            const double* __restrict__ lse, const int32_t* __restrict__ count,
                                                            const float* __restrict__ grad_loss, int64_t n_rows,
                                                            const int32_t* __restrict__ n_valid, int classes, float smoothing,
                                                            bool vec4, float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int stride = tile_stride(classes);
  float* tile = reinterpret_cast<float*>(smem);
  const int t = threadIdx.x;
  const int64_t present = present_rows(n_valid, n_rows);
  const int64_t r0 = (int64_t)blockIdx.x * kChunk, r = r0 + t;
  const int rows_buf = (int)min((int64_t)kChunk, n_rows - r0);  // rows of the buffer in this chunk: all of them are written
  float* out0 = grad + r0 * classes;
  if (r0 >= present) {  // (the whole workgroup)
    for (int e = t; e < rows_buf * classes; e += kChunk) out0[e] = 0.f;
    return;
  }
  const int rows = (int)min((int64_t)kChunk, present - r0);
  if (STAGED) {
    stage_rows(logits + r0 * classes, rows * classes, classes, stride, tile, vec4);
    __syncthreads();
  }
  if (t < rows_buf) {
    bool ok = false;
    int64_t label = -1;
    if (t < rows) {
      label = load_label(labels, label_bits, r);
      ok = row_counts(label, classes, counted);
    }
    const float* x = STAGED ? tile + t * stride : logits + r * classes;
    float* out = STAGED ? tile + t * stride : grad + r * classes;  // (staged: the row is overwritten in place)
    if (ok) {
      const double eps = (double)smoothing, k = (double)classes;
      const double g = (double)*grad_loss, cnt = (double)max(*count, 1), l = lse[r];
      const double q_other = eps / k, q_label = q_other + (1.0 - eps);
      for (int c = 0; c < classes; ++c) out[c] = seg_grad(x[c], l, c == (int)label ? q_label : q_other, g, cnt);
    } else {
      for (int c = 0; c < classes; ++c) out[c] = 0.f;
    }
  }
  if (STAGED) {
    __syncthreads();
    unstage_rows(tile, out0, rows_buf * classes, classes, stride, vec4);
  }
}

// the checks both entry points and the query share
int seg_head_shape(int64_t n_rows, int32_t classes) {
  if (n_rows < 0 || classes < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (classes > kMaxClasses) return SE3_ERR_UNSUPPORTED;
  if (n_rows > ((1ll << 31) - 1) / classes) return SE3_ERR_UNSUPPORTED;  // n_rows * classes >= 2^31
  return SE3_OK;
}

int seg_head_args(int64_t n_rows, int32_t classes, int32_t label_bits, float smoothing) {
  if (n_rows < 0 || classes < 1 || (label_bits != 32 && label_bits != 64) || !(smoothing >= 0.f && smoothing <= 1.f))
    return SE3_ERR_INVALID_ARGUMENT;
  return seg_head_shape(n_rows, classes);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" size_t se3_seg_head_workspace_bytes(int64_t n_rows, int32_t classes) {
  if (seg_head_shape(n_rows, classes) != SE3_OK) return 0;
  return seg_head_layout(n_rows, classes).total;
}

extern "C" int se3_seg_loss_fwd(const float* logits, const void* labels, int32_t label_bits, const uint8_t* counted,
                                int64_t n_rows, const int32_t* n_valid, int32_t classes, float smoothing, float* loss,
                                int32_t* count, double* lse, int64_t* tallies, void* workspace, size_t workspace_bytes,
                                void* stream_) {
  if (int rc = seg_head_args(n_rows, classes, label_bits, smoothing)) return rc;
  if (!loss || !count || !workspace || (n_rows > 0 && (!logits || !labels))) return SE3_ERR_INVALID_ARGUMENT;
  const SegHeadLayout l = seg_head_layout(n_rows, classes);
  if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* w = (char*)workspace;
  double* part_sum = (double*)(w + l.sums);
  int32_t* part_count = (int32_t*)(w + l.counts);
  int32_t* part_hist = (int32_t*)(w + l.hists);
  const bool want_hist = tallies != nullptr;
  if (n_rows > 0) {
    const dim3 grid((unsigned)chunks_of(n_rows)), block(kChunk);
    const size_t tail = kChunk * sizeof(double) + 3 * (size_t)classes * sizeof(int);
    if (classes <= kTileClasses)
      hipLaunchKernelGGL(seg_loss_rows_kernel<true>, grid, block, tile_bytes(classes) + tail, stream, logits, labels, label_bits,
                         counted, n_rows, n_valid, classes, smoothing, lse, want_hist, aligned16(logits), part_sum, part_count,
                         part_hist);
    else
      hipLaunchKernelGGL(seg_loss_rows_kernel<false>, grid, block, tail, stream, logits, labels, label_bits, counted, n_rows,
                         n_valid, classes, smoothing, lse, want_hist, false, part_sum, part_count, part_hist);
  }
  const unsigned blocks = 1u + (want_hist ? (unsigned)((3 * classes + 255) / 256) : 0u);
  hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(blocks), dim3(256), 0, stream, part_sum, part_count, part_hist, n_rows, n_valid,
                     classes, loss, count, tallies);
  return check_launch();
}

extern "C" int se3_seg_loss_bwd(const float* logits, const void* labels, int32_t label_bits, const uint8_t* counted,
                                const double* lse, const int32_t* count, const float* grad_loss, int64_t n_rows,
                                const int32_t* n_valid, int32_t classes, float smoothing, float* grad_logits, void* stream_) {
  if (int rc = seg_head_args(n_rows, classes, label_bits, smoothing)) return rc;
  if (!count || !grad_loss || (n_rows > 0 && (!logits || !labels || !lse || !grad_logits))) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return SE3_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)chunks_of(n_rows)), block(kChunk);
  if (classes <= kTileClasses)
    hipLaunchKernelGGL(seg_loss_grad_kernel<true>, grid, block, tile_bytes(classes), stream, logits, labels, label_bits, counted,
                       lse, count, grad_loss, n_rows, n_valid, classes, smoothing, aligned16(logits) && aligned16(grad_logits),
                       grad_logits);
  else
    hipLaunchKernelGGL(seg_loss_grad_kernel<false>, grid, block, 0, stream, logits, labels, label_bits, counted, lse, count,
                       grad_loss, n_rows, n_valid, classes, smoothing, false, grad_logits);
  return check_launch();
}
