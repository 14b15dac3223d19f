// Farthest-point sampling for gfx950 (include/se3conv_fps.h holds the contract; replaces what pc/FPSSubSample.py of the
// reference asks of torch_cluster.fps).
//
//   fps_prepare_kernel   one workgroup: batch ids sorted and in range?  element boundaries (binary search in the sorted
//                        ids), sample counts, their exclusive prefix sum, info
//   fps_fill_tail_kernel ids / d2_at_pick behind min(M, capacity)
//   fps_sample_kernel    ONE workgroup of 1024 threads per element, the sequential loop over picks inside it; no workgroup
//                        waits for another one
//
// A pick costs: every lane's update of its rows' `mind` and its local argmax, a cross-lane max of one 64-bit key per
// wavefront (DPP inside a row of 16 lanes, two ds_bpermute steps across rows), one barrier, and a 16-slot LDS read.  The
// key is `mind` bits << 32 | ~row: squared distances are >= 0, so their bits order like the numbers, and the complemented
// index makes an unsigned max pick the LOWEST row among equal distances.  The winner's coordinates travel with the key
// through the wavefront's LDS slot, so the loop of the resident form touches global memory only to store its picks.
#include "common.h"
#include "../../include/se3conv_fps.h"

namespace se3 {

namespace {

constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsRows = SE3_FPS_RESIDENT_MAX / kFpsThreads;  // rows a thread keeps in registers
constexpr int kFpsUnroll = 4;                                 // rows per trip of the streaming form's loop
static_assert(kFpsRows * kFpsThreads == SE3_FPS_RESIDENT_MAX && kFpsWaves == 16, "the reduction reads 16 slots, one DPP row");

struct FpsLayout {
  size_t elem_starts, mind, total;  // int32 [n_batches+1]; fp32 [n_rows] (the streaming form's mind, -1 = picked)
};
inline FpsLayout fps_layout(int64_t n_rows, int32_t n_batches) {
  FpsLayout l;
  l.elem_starts = 0;
  l.mind = align_up(sizeof(int32_t) * ((size_t)n_batches + 1), 256);
  l.total = l.mind + align_up(sizeof(float) * (size_t)(n_rows > 0 ? n_rows : 1), 256);
  return l;
}

// first position in ids[0, n) whose value is >= v (ids non-decreasing)
__device__ __forceinline__ int fps_lower_bound(const int32_t* __restrict__ ids, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kFpsThreads) void fps_prepare_kernel(const int32_t* __restrict__ batch_ids, int64_t n_rows,
                                                                  const int32_t* __restrict__ n_valid, int32_t n_batches,
                                                                  float ratio, int64_t capacity, int32_t* __restrict__ elem_starts,
                                                                  int32_t* __restrict__ out_starts, int32_t* __restrict__ info) {
  __shared__ int wave_sums[kFpsWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int n = (int)n_rows;
  if (n_valid) n = min(max(*n_valid, 0), n);
  int bad = 0;
  for (int64_t i = t; i < n; i += kFpsThreads) {  // (64-bit counters: n may be one stride short of 2^31)
    const int v = batch_ids[i];
    bad |= (v < 0) | (v >= n_batches);
    if (i > 0) bad |= batch_ids[i - 1] > v;
  }
  bad = __syncthreads_or(bad) ? 1 : 0;
  int carry = 0;  // samples of the elements before this chunk (uniform)
  for (int64_t base = 0; base < n_batches; base += kFpsThreads) {
    const int64_t b = base + t;
    int m = 0;
    if (b < n_batches) {
      int lo = 0;
      if (!bad) {
        lo = fps_lower_bound(batch_ids, n, (int)b);
        const int nb = (b + 1 < n_batches ? fps_lower_bound(batch_ids, n, (int)b + 1) : n) - lo;
        m = min(nb, (int)ceilf(__fmul_rn((float)nb, ratio)));
      }
      elem_starts[b] = lo;
    }
    int incl = m;  // inclusive scan: inside the wavefront, then over the wavefronts' sums
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kFpsWaves; ++w) {
      const int s = wave_sums[w];
      before += w < wave ? s : 0;
      total += s;
    }
    if (b < n_batches) out_starts[b] = carry + before + incl - m;
    carry += total;
    __syncthreads();  // wave_sums is written again by the next chunk
  }
  if (t == 0) {
    elem_starts[n_batches] = bad ? 0 : n;
    out_starts[n_batches] = carry;
    info[0] = carry;
    info[1] = (int64_t)carry > capacity;
    info[2] = bad;
  }
}

__global__ void fps_fill_tail_kernel(const int32_t* __restrict__ info, int64_t capacity, int32_t* __restrict__ ids,
                                     float* __restrict__ d2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= capacity || i < (int64_t)info[0]) return;
  ids[i] = -1;
  if (d2) d2[i] = -1.0f;
}

// ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded on its own.  hipcc contracts a * b + c into an fma by default, and
// also through __fmul_rn / __fadd_rn (plain operators in headers compiled with contraction on): the operators below stand
// under a pragma that switches contraction off for this function, and the fp32 result is that of numpy.
__device__ __forceinline__ float fps_d2(float x, float y, float z, float px, float py, float pz) {
#pragma clang fp contract(off)
  const float dx = x - px, dy = y - py, dz = z - pz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

template <int CTRL>
__device__ __forceinline__ uint64_t fps_dpp_max(uint64_t k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, 0xF, 0xF, false);
  const uint64_t o = ((uint64_t)hi << 32) | lo;
  return o > k ? o : k;
}
// max over each row of 16 lanes, in every lane of the row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror (every lane is active where this is called)
__device__ __forceinline__ uint64_t fps_row_max(uint64_t k) {
  k = fps_dpp_max<0xB1>(k);
  k = fps_dpp_max<0x4E>(k);
  k = fps_dpp_max<0x141>(k);
  return fps_dpp_max<0x140>(k);
}
__device__ __forceinline__ uint64_t fps_wave_max(uint64_t k) {
  k = fps_row_max(k);
#pragma unroll
  for (int m = 16; m < 64; m <<= 1) {
    const uint64_t o = __shfl_xor(k, m);
    k = o > k ? o : k;
  }
  return k;
}

struct FpsSlot {
  uint64_t key;
  float x, y, z, pad;
};

struct FpsBest {  // a lane's best unmarked row: key 0 = none
  uint64_t key = 0;
  float x = 0.f, y = 0.f, z = 0.f;
  // `mind` < 0 marks a picked (or absent) row
  __device__ __forceinline__ void offer(float mind, int row, float px, float py, float pz) {
    const uint64_t k = mind >= 0.f ? ((uint64_t)__float_as_uint(mind) << 32) | (uint32_t)~row : 0ull;
    if (k > key) key = k, x = px, y = py, z = pz;
  }
};

// The workgroup's winner of one pick: its row inside the element, its mind and its coordinates, in every thread.  ONE
// barrier: pick j writes slot set j & 1, and whoever writes that set again (pick j + 2) has passed the barrier of pick
// j + 1, which every thread reaches only after its reads here.
__device__ __forceinline__ void fps_winner(const FpsBest& best, FpsSlot (*slots)[kFpsWaves], int set, int lane, int wave,
                                           int& p, float& dwin, float& px, float& py, float& pz) {
  const uint64_t wk = fps_wave_max(best.key);
  // keys of unmarked rows are distinct, so one lane matches; in a wavefront without an unmarked row all match with key
  // 0, which never wins (a pick is only searched while unmarked rows are left)
  if (best.key == wk) slots[set][wave] = FpsSlot{wk, best.x, best.y, best.z, 0.f};
  __syncthreads();
  const uint64_t bk = fps_row_max(slots[set][lane & (kFpsWaves - 1)].key);
  p = (int)~(uint32_t)bk;
  dwin = __uint_as_float((uint32_t)(bk >> 32));
  const FpsSlot& s = slots[set][(p & (kFpsThreads - 1)) >> 6];  // thread t owns rows t, t + 1024, ...
  px = s.x, py = s.y, pz = s.z;
}

__global__ __launch_bounds__(kFpsThreads) void fps_sample_kernel(const float* __restrict__ pts,
                                                                 const int32_t* __restrict__ elem_starts,
                                                                 const int32_t* __restrict__ out_starts,
                                                                 const float* __restrict__ start_u, int64_t capacity,
                                                                 int32_t* __restrict__ ids, float* __restrict__ d2_at_pick,
                                                                 float* __restrict__ mind_ws) {
  __shared__ FpsSlot slots[2][kFpsWaves];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r0 = elem_starts[b], nb = elem_starts[b + 1] - r0;
  const int o0 = out_starts[b], mb = out_starts[b + 1] - o0;
  // positions >= capacity are not written: the loop stops there, and what it wrote is the untruncated call's prefix
  const int64_t room = capacity - (int64_t)o0;
  const int picks = (int)(room < (int64_t)mb ? room : (int64_t)mb);
  if (picks <= 0 || nb <= 0) return;  // (uniform: before any barrier)
  int p = 0;
  if (start_u) {
    const float u = start_u[b];
    p = u >= 0.f ? (int)fminf(floorf(__fmul_rn(u, (float)nb)), 2.0e9f) : 0;
    p = min(max(p, 0), nb - 1);
  }
  const float* __restrict__ ept = pts + (int64_t)r0 * 3;
  float px = ept[(int64_t)p * 3], py = ept[(int64_t)p * 3 + 1], pz = ept[(int64_t)p * 3 + 2];
  float dwin = __builtin_inff();
  int32_t* __restrict__ out_ids = ids + o0;
  float* __restrict__ out_d2 = d2_at_pick ? d2_at_pick + o0 : nullptr;

  if (nb <= SE3_FPS_RESIDENT_MAX) {
    float x[kFpsRows], y[kFpsRows], z[kFpsRows], mind[kFpsRows];
#pragma unroll
    for (int k = 0; k < kFpsRows; ++k) {
      const int i = t + k * kFpsThreads;
      const bool in = i < nb;
      x[k] = in ? ept[(int64_t)i * 3] : 0.f;
      y[k] = in ? ept[(int64_t)i * 3 + 1] : 0.f;
      z[k] = in ? ept[(int64_t)i * 3 + 2] : 0.f;
      mind[k] = in ? __builtin_inff() : -1.0f;
    }
    for (int j = 0;; ++j) {
      if (t == 0) {
        out_ids[j] = r0 + p;
        if (out_d2) out_d2[j] = dwin;
      }
      if (j + 1 == picks) break;
      FpsBest best;
#pragma unroll
      for (int k = 0; k < kFpsRows; ++k) {
        const int i = t + k * kFpsThreads;
        const float m = mind[k];
        const float d = fminf(m, fps_d2(x[k], y[k], z[k], px, py, pz));
        mind[k] = (m < 0.f || i == p) ? -1.0f : d;
        best.offer(mind[k], i, x[k], y[k], z[k]);
      }
      fps_winner(best, slots, j & 1, lane, wave, p, dwin, px, py, pz);
    }
  } else {
    float* __restrict__ emind = mind_ws + r0;
    for (int j = 0;; ++j) {
      if (t == 0) {
        out_ids[j] = r0 + p;
        if (out_d2) out_d2[j] = dwin;
      }
      if (j + 1 == picks) break;
      FpsBest best;
      // row i is read and written by this thread alone; the first pass reads nothing the caller left in the workspace
      auto row = [&](int i, float xi, float yi, float zi, float m) {
        const float d = fminf(m, fps_d2(xi, yi, zi, px, py, pz));
        const float nm = (m < 0.f || i == p) ? -1.0f : d;
        emind[i] = nm;
        best.offer(nm, i, xi, yi, zi);
      };
      int64_t i = t;  // (64-bit: an element may end one stride short of 2^31)
      // four rows per trip, their sixteen loads in flight together: one workgroup has only its own loads to wait for
      for (; i + (kFpsUnroll - 1) * kFpsThreads < nb; i += kFpsUnroll * kFpsThreads) {
        float xs[kFpsUnroll], ys[kFpsUnroll], zs[kFpsUnroll], ms[kFpsUnroll];
#pragma unroll
        for (int u = 0; u < kFpsUnroll; ++u) {
          const int64_t r = i + u * kFpsThreads;
          xs[u] = ept[r * 3], ys[u] = ept[r * 3 + 1], zs[u] = ept[r * 3 + 2];
          ms[u] = j == 0 ? __builtin_inff() : emind[r];
        }
#pragma unroll
        for (int u = 0; u < kFpsUnroll; ++u) row((int)i + u * kFpsThreads, xs[u], ys[u], zs[u], ms[u]);
      }
      for (; i < nb; i += kFpsThreads)
        row((int)i, ept[i * 3], ept[i * 3 + 1], ept[i * 3 + 2], j == 0 ? __builtin_inff() : emind[i]);
      fps_winner(best, slots, j & 1, lane, wave, p, dwin, px, py, pz);
    }
  }
}

}  // namespace

}  // namespace se3

using namespace se3;

extern "C" size_t se3_fps_workspace_bytes(int64_t n_rows, int32_t n_batches) {
  if (n_rows < 0 || n_rows >= (1ll << 31) || n_batches < 1) return 0;
  return fps_layout(n_rows, n_batches).total;
}

extern "C" int se3_fps(const float* pts, const int32_t* batch_ids, int64_t n_rows, const int32_t* n_valid, int32_t n_batches,
                       float ratio, const float* start_u, int64_t capacity, int32_t* ids, float* d2_at_pick,
                       int32_t* out_starts, int32_t* info, void* workspace, size_t workspace_bytes, void* stream_) {
  if (n_rows < 0 || n_batches < 1 || capacity < 0 || !ids || !out_starts || !info || !workspace) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows > 0 && (!pts || !batch_ids)) return SE3_ERR_INVALID_ARGUMENT;
  if (!(ratio > 0.f && ratio <= 1.f)) return SE3_ERR_INVALID_ARGUMENT;  // (NaN fails both comparisons)
  if (n_rows >= (1ll << 31) || capacity >= (1ll << 31)) return SE3_ERR_UNSUPPORTED;
  const FpsLayout lay = fps_layout(n_rows, n_batches);
  if (workspace_bytes < lay.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  int32_t* elem_starts = (int32_t*)((char*)workspace + lay.elem_starts);
  float* mind = (float*)((char*)workspace + lay.mind);
  hipLaunchKernelGGL(fps_prepare_kernel, dim3(1), dim3(kFpsThreads), 0, stream, batch_ids, n_rows, n_valid, n_batches, ratio,
                     capacity, elem_starts, out_starts, info);
  if (capacity > 0)
    hipLaunchKernelGGL(fps_fill_tail_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, stream, info, capacity, ids,
                       d2_at_pick);
  hipLaunchKernelGGL(fps_sample_kernel, dim3((unsigned)n_batches), dim3(kFpsThreads), 0, stream, pts, elem_starts, out_starts,
                     start_u, capacity, ids, d2_at_pick, mind);
  return check_launch();
}
