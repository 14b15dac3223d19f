// The edge list of a k-NN id table (include/se3conv_knn_edges.h): `[n_rows, k]` ids with -1 padding -> the sample-major
// `(neighbors [capacity,2], ends [n_rows], info [2])` triple of se3_ball_query_bounded, the edge count staying on the device.
//
//   count   one thread per row: the length of the row's valid prefix (0 for an absent row)
//   scan    hipcub::DeviceScan::InclusiveSum of the counts -> the unclamped inclusive end offsets
//   store   one thread per table entry: (row, id) to its offset if it is inside the row's prefix and the buffer; the row's
//           first thread writes the clamped `ends` entry, the table's first thread `info`
//
// No atomics: the list is a pure function of the table and the row-count word.
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "../../include/se3conv_knn_edges.h"

namespace se3 {
namespace {

struct KnnEdgesLayout {
  size_t counts, raw, temp, temp_bytes, total;
};

KnnEdgesLayout knn_edges_layout(int64_t n_rows) {
  const size_t n = (size_t)(n_rows > 0 ? n_rows : 1);
  KnnEdgesLayout l{};
  l.counts = 0;
  l.raw = align_up(n * sizeof(int32_t), 256);
  l.temp = l.raw + align_up(n * sizeof(int32_t), 256);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, l.temp_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  l.total = l.temp + align_up(l.temp_bytes, 256);
  return l;
}

__global__ __launch_bounds__(256) void knn_edges_count_kernel(const int32_t* __restrict__ ids, int64_t n_rows,
                                                              const int32_t* __restrict__ n_valid, int k,
                                                              int32_t* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  int c = 0;
  if (r < present_rows(n_valid, n_rows)) {  // (an absent row of the table is not read)
    const int32_t* row = ids + r * k;
    while (c < k && row[c] >= 0) ++c;
  }
  counts[r] = c;
}

__global__ __launch_bounds__(256) void knn_edges_store_kernel(const int32_t* __restrict__ ids, int64_t n_rows, int k,
                                                              const int32_t* __restrict__ counts,
                                                              const int32_t* __restrict__ raw, int limit,
                                                              int32_t* __restrict__ neighbors, int32_t* __restrict__ ends,
                                                              int32_t* __restrict__ info) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * k) return;
  const int64_t r = t / k;
  const int j = (int)(t - r * k);
  const int end = raw[r], cnt = counts[r];
  if (j < cnt) {  // (cnt = 0 for an absent row: nothing of it is read)
    const int pos = end - cnt + j;
    if (pos < limit) {
      neighbors[2 * (int64_t)pos] = (int32_t)r;
      neighbors[2 * (int64_t)pos + 1] = ids[t];
    }
  }
  if (j == 0) ends[r] = min(end, limit);
  if (t == 0) {
    const int total = raw[n_rows - 1];
    info[0] = total;
    info[1] = total > limit ? 1 : 0;
  }
}

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" size_t se3_knn_edges_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows >= (1ll << 31)) return 0;
  return knn_edges_layout(n_rows).total;
}

extern "C" int se3_knn_edges_bounded(const int32_t* ids, int64_t n_rows, const int32_t* n_valid, int32_t k, int64_t capacity,
                                     int32_t* neighbors, int32_t* ends, int32_t* info, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows < 0 || k < 1 || capacity < 0 || capacity >= (1ll << 31) || !info) return SE3_ERR_INVALID_ARGUMENT;
  if (k > 64 || n_rows >= (1ll << 31) || n_rows * k >= (1ll << 31)) return SE3_ERR_UNSUPPORTED;
  // no row, no thread: `info`, which the store pass writes, is filled here
  if (n_rows == 0) return launch_fill_words(info, 0u, 2, stream);
  if (!ids || !ends || !workspace || (capacity > 0 && !neighbors)) return SE3_ERR_INVALID_ARGUMENT;
  const KnnEdgesLayout l = knn_edges_layout(n_rows);
  if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  int32_t* counts = (int32_t*)(ws + l.counts);
  int32_t* raw = (int32_t*)(ws + l.raw);
  hipLaunchKernelGGL(knn_edges_count_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream, ids, n_rows,
                     n_valid, (int)k, counts);
  size_t temp_bytes = l.temp_bytes;
  if (hipcub::DeviceScan::InclusiveSum(ws + l.temp, temp_bytes, counts, raw, (int)n_rows, stream) != hipSuccess)
    return SE3_ERR_LAUNCH;
  const int64_t entries = n_rows * k;
  hipLaunchKernelGGL(knn_edges_store_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, ids, n_rows,
                     (int)k, counts, raw, (int)capacity, neighbors, ends, info);
  return check_launch();
}
