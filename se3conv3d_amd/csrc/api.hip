// extern "C" entry points of the fused operator + the API-parity ops (see include/se3conv.h).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "../../include/se3conv_forms.h"

namespace se3 {

// ---- the forms query (common.h): while `t_forms` is set on a thread the entry points launch nothing and the launchers
// report which form they chose ---------------------------------------------------------------------------------------------
namespace {
struct FormSink { std::string lines, tag; int n_cu; };
thread_local FormSink* t_forms = nullptr;
}  // namespace
bool forms_only() { return t_forms != nullptr; }
int forms_cu_count() { return t_forms ? t_forms->n_cu : 0; }
const Switches& switches() {
  static const Switches sw = [] {
    Switches v{};
    v.no_t24 = getenv("SE3_NO_T24") != nullptr;
    v.no_pair = getenv("SE3_NO_PAIR") != nullptr;
    v.pg_single = getenv("SE3_PG_SINGLE") != nullptr;
    v.tr_merge_sort = getenv("SE3_TR_MERGE_SORT") != nullptr;
    const char* dx = getenv("SE3_DX_PATH");
    v.dx_path = dx ? atoi(dx) : -1;
    const char* es = getenv("SE3_EDGE_STREAM");  // n > 0: n items; anything else: never
    v.edge_stream_min_items = es ? (atoi(es) > 0 ? atoi(es) : INT32_MAX) : 4096;
    // a second field of the same variable, "<dx>,dense=<n>", gates the shared launch of backward's dense products (the other
    // decision of plan_bwd): n > 0: levels of up to n rows; anything else: never.  (<dx> = -1 is the cost model, as without it.)
    const char* ds = dx ? strstr(dx, "dense=") : nullptr;
    v.dense_share_rows = ds ? (atoll(ds + 6) > 0 ? atoll(ds + 6) : 0) : kDenseShareRows;
    return v;
  }();
  return sw;
}
int form_report(const char* tag, const char* fmt, ...) {  // tag == nullptr: a launch inside the stage reported last
  if (!t_forms) return SE3_OK;
  if (tag) t_forms->tag = tag;
  char name[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(name, sizeof(name), fmt, ap);
  va_end(ap);
  t_forms->lines += t_forms->tag + ":" + name + "\n";
  return SE3_OK;
}

namespace {

// dst[c][r] = src[r][c]   (src [rows, cols])
__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i / rows), r = (int)(i % rows);
    dst[i] = src[(int64_t)r * cols + c];
  }
}

// w2[(o*K + k), i] = w[i, k, o]
__global__ void permute_weights_oki_kernel(const float* __restrict__ w, float* __restrict__ w2, int c_in, int kb,
                                           int c_out) {
  const int64_t total = (int64_t)c_in * kb * c_out;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx % c_in);
    const int ok = (int)(idx / c_in);
    const int k = ok % kb, o = ok / kb;
    w2[idx] = w[((int64_t)i * kb + k) * c_out + o];
  }
}

// one block per output element: 256 threads stride over the per-block partials, then tree-reduce
__global__ __launch_bounds__(256) void reduce_param_partials_kernel(const float* __restrict__ partials, int n_partials,
                                                                    float* __restrict__ grad_axes,
                                                                    float* __restrict__ grad_biases, float scale) {
  __shared__ float red[256];
  const int i = blockIdx.x;
  float s = 0.f;
  for (int p = threadIdx.x; p < n_partials; p += 256) s += partials[(int64_t)p * kDescExt * kBasis + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (i < SE3_DESC_DIMS * kBasis) {
      if (grad_axes) grad_axes[i] = red[0] * scale;
    } else if (grad_biases) {
      grad_biases[i - SE3_DESC_DIMS * kBasis] = red[0] * scale;
    }
  }
}

// ---- API-parity kernels (not on the fused path) ------------------------------------------------

// Rotation matrix (row-major m[9]) -> real-part-first quaternion as RotationFunctions.py:91-151 computes it: the four
// candidates q * 2 q_r, q * 2 q_i, ..., the one with the largest |component| is divided out (denominator floored at 0.1).
__device__ __forceinline__ void matrix_to_quaternion(const float m[9], float q[4]) {
  const float t[4] = {1.0f + m[0] + m[4] + m[8], 1.0f + m[0] - m[4] - m[8], 1.0f - m[0] + m[4] - m[8],
                      1.0f - m[0] - m[4] + m[8]};
  float qa[4];
  int best = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    qa[i] = t[i] > 0.f ? sqrtf(t[i]) : 0.f;
    if (qa[i] > qa[best]) best = i;  // first maximum, as torch.argmax
  }
  const float c[4][4] = {{qa[0] * qa[0], m[7] - m[5], m[2] - m[6], m[3] - m[1]},
                         {m[7] - m[5], qa[1] * qa[1], m[3] + m[1], m[2] + m[6]},
                         {m[2] - m[6], m[3] + m[1], qa[2] * qa[2], m[5] + m[7]},
                         {m[3] - m[1], m[6] + m[2], m[7] + m[5], qa[3] * qa[3]}};
  const float den = 2.0f * fmaxf(qa[best], 0.1f);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = (best == 0 ? c[0][i] : best == 1 ? c[1][i] : best == 2 ? c[2][i] : c[3][i]) / den;
}

// get_rot_tenors materialised (PNEConvLayerRotEquiv.py:62-128): one thread per (edge, a, b).  REL = representation of
// the relative rotation R_out^T R_in (get_relative_rot, RotationFunctions.py:549-600): 0 "6D" (its first two rows, D = 9),
// 1 "matrix" (all nine entries, D = 12), 2 "quaternion" (D = 7).
template <int REL>
__global__ void rot_tensors_kernel(const float* __restrict__ pts_in, const float* __restrict__ pts_out,
                                   const float* __restrict__ frames_in, const float* __restrict__ frames_out,
                                   const int32_t* __restrict__ neighbors, const int32_t* __restrict__ ends,
                                   const float* __restrict__ rho_p, int64_t n_edges, int f_in, int f_out,
                                   float* __restrict__ desc, int32_t* __restrict__ fe_neighbors) {
  constexpr int D = REL == 0 ? 9 : (REL == 1 ? 12 : 7);
  const float rho = *rho_p;
  const int ff = f_in * f_out;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_edges * ff;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / ff;
    const int ab = (int)(t - e * ff);
    const int a = ab / f_in, b = ab % f_in;
    const int s = neighbors[e * 2], p = neighbors[e * 2 + 1];
    const int start = s > 0 ? ends[s - 1] : 0;
    const int deg = ends[s] - start;
    const int64_t idx = (int64_t)ff * start + (int64_t)a * deg * f_in + (e - start) * f_in + b;
    float x[3], y[3], ri[9], ro[9], d[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = pts_in[(int64_t)p * 3 + i], y[i] = pts_out[(int64_t)s * 3 + i];
#pragma unroll
    for (int i = 0; i < 9; ++i)
      ri[i] = frames_in[((int64_t)p * f_in + b) * 9 + i], ro[i] = frames_out[((int64_t)s * f_out + a) * 9 + i];
    edge_descriptor(x, ri, y, ro, rho, d);
    if constexpr (REL == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) desc[idx * 9 + i] = d[i];
    } else {
      float rel[9];  // d[3..8] are rows 0, 1 of R_out^T R_in; row 2 the same way
#pragma unroll
      for (int i = 0; i < 6; ++i) rel[i] = d[3 + i];
#pragma unroll
      for (int c = 0; c < 3; ++c) rel[6 + c] = ro[2] * ri[c] + ro[5] * ri[3 + c] + ro[8] * ri[6 + c];
#pragma unroll
      for (int i = 0; i < 3; ++i) desc[idx * D + i] = d[i];
      if constexpr (REL == 1) {
#pragma unroll
        for (int i = 0; i < 9; ++i) desc[idx * D + 3 + i] = rel[i];
      } else {
        float q[4];
        matrix_to_quaternion(rel, q);
#pragma unroll
        for (int i = 0; i < 4; ++i) desc[idx * D + 3 + i] = q[i];
      }
    }
    fe_neighbors[idx * 2] = s * f_out + a;
    fe_neighbors[idx * 2 + 1] = p * f_in + b;
  }
}

__global__ void rot_tensor_ends_kernel(const int32_t* __restrict__ ends, int64_t n_out, int f_in, int f_out,
                                       int32_t* __restrict__ fe_ends) {
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < n_out * f_out;
       m += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = m / f_out;
    const int a = (int)(m - s * f_out);
    const int start = s > 0 ? ends[s - 1] : 0;
    const int deg = ends[s] - start;
    fe_ends[m] = f_in * f_out * start + (a + 1) * deg * f_in;
  }
}

// T[m,c,k] = sum_e basis[e,k] feat[src(e),c]  (feat_basis_proj.cu:24-123): one block per row,
// thread = (channel group, k); generic in C and K.
__global__ __launch_bounds__(256) void feat_basis_proj_kernel(const float* __restrict__ basis,
                                                              const float* __restrict__ feat,
                                                              const int32_t* __restrict__ neighbors,
                                                              const int32_t* __restrict__ ends, int channels, int kb,
                                                              float* __restrict__ out) {
  const int64_t m = blockIdx.x;
  const int start = m > 0 ? ends[m - 1] : 0, end = ends[m];
  const int k = threadIdx.x % kb, cg = threadIdx.x / kb, ncg = blockDim.x / kb;
  for (int c = cg; c < channels; c += ncg) {
    float acc = 0.f;
    for (int e = start; e < end; ++e)
      acc += basis[(int64_t)e * kb + k] * feat[(int64_t)neighbors[(int64_t)e * 2 + 1] * channels + c];
    out[(m * channels + c) * kb + k] = acc;
  }
}

__device__ __forceinline__ int row_of_edge(const int32_t* __restrict__ ends, int64_t n_rows, int64_t e) {
  int64_t lo = 0, hi = n_rows;  // first row with ends[row] > e
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ends[mid] <= e) lo = mid + 1; else hi = mid;
  }
  return (int)lo;
}

// gBasis[e,k] = sum_c gT[m,c,k] feat[p,c]   (feat_basis_proj_grads.cu:113-126)
__global__ void feat_basis_proj_grad_basis_kernel(const float* __restrict__ feat, const int32_t* __restrict__ neighbors,
                                                  const int32_t* __restrict__ ends, const float* __restrict__ grad_t,
                                                  int64_t n_edges, int64_t n_rows, int channels, int kb,
                                                  float* __restrict__ g_basis) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_edges * kb;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / kb;
    const int k = (int)(t - e * kb);
    const int64_t m = row_of_edge(ends, n_rows, e);
    const float* f = feat + (int64_t)neighbors[e * 2 + 1] * channels;
    const float* g = grad_t + m * channels * kb + k;
    float acc = 0.f;
    for (int c = 0; c < channels; ++c) acc += g[(int64_t)c * kb] * f[c];
    g_basis[t] = acc;
  }
}

// gFeat[p,c] += sum_k gT[m,c,k] basis[e,k]   (feat_basis_proj_grads.cu:129-140; float atomics as there)
__global__ void feat_basis_proj_grad_feat_kernel(const float* __restrict__ basis, const int32_t* __restrict__ neighbors,
                                                 const int32_t* __restrict__ ends, const float* __restrict__ grad_t,
                                                 int64_t n_edges, int64_t n_rows, int channels, int kb,
                                                 float* __restrict__ g_feat) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_edges * channels;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / channels;
    const int c = (int)(t - e * channels);
    const int64_t m = row_of_edge(ends, n_rows, e);
    const float* g = grad_t + (m * channels + c) * kb;
    const float* b = basis + e * kb;
    float acc = 0.f;
    for (int k = 0; k < kb; ++k) acc += g[k] * b[k];
    atomicAdd(&g_feat[(int64_t)neighbors[e * 2 + 1] * channels + c], acc);
  }
}

inline unsigned grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > 1 << 20) b = 1 << 20;
  return (unsigned)b;
}

bool shape_ok(const se3conv_shape* s) {
  return s && s->n_in >= 0 && s->n_out >= 0 && s->n_edges >= 0 && s->f_in >= 1 && s->f_out >= 1 && s->c_in >= 1 &&
         s->c_out >= 1 && s->num_basis >= 1 &&
         (s->precision == SE3_PRECISION_FP32 || s->precision == SE3_PRECISION_BF16X3 ||
          s->precision == SE3_PRECISION_BF16X3_T16);
}
int shape_supported(const se3conv_shape* s) {
  if (s->num_basis != kBasis) return SE3_ERR_UNSUPPORTED;  // every shipped config uses K = 32
  if (s->n_in * s->f_in >= (1ll << 31) || s->n_out * s->f_out >= (1ll << 31) ||
      s->n_edges * s->f_in * s->f_out >= (1ll << 31))
    return SE3_ERR_UNSUPPORTED;  // row / frame-edge ids are int32 inside the kernels
  if (s->n_in * s->f_in * s->c_in >= (1ll << 29) || s->n_out * s->f_out * s->c_out >= (1ll << 29) ||
      s->n_in * s->f_in >= (1ll << 25) || s->n_out * s->f_out >= (1ll << 25))
    return SE3_ERR_UNSUPPORTED;  // gathered operands (< 2 GB) and the 64-byte geometry records are addressed with 32-bit byte offsets
  return SE3_OK;
}

// The two views of a call's graph for the edge kernels.  Without pointers they are the shape alone, which is all the
// plans below ask the kernels' `*_applicable` / `*_rows` predicates about.
EdgeGeom forward_geom(const se3conv_shape* s, const float* pts_in = nullptr, const float* pts_out = nullptr,
                      const float* frames_in = nullptr, const float* frames_out = nullptr, const int32_t* neighbors = nullptr,
                      const int32_t* ends = nullptr) {
  EdgeGeom g{};
  g.ctr_pts = pts_out, g.ctr_frames = frames_out, g.nb_pts = pts_in, g.nb_frames = frames_in;
  g.nbr = neighbors, g.nbr_stride = 2, g.nbr_offset = 1, g.ends = ends;
  g.n_ctr = s->n_out, g.f_ctr = s->f_out, g.f_nb = s->f_in, g.transposed = 0;
  g.n_nb = s->n_in;
  g.n_edges = s->n_edges;
  return g;
}
// transposed graph: centre = input point, edges lead to output points (feature gradient)
EdgeGeom transposed_geom(const se3conv_shape* s, const float* pts_in = nullptr, const float* pts_out = nullptr,
                         const float* frames_in = nullptr, const float* frames_out = nullptr, const int32_t* t_samples = nullptr,
                         const int32_t* t_ends = nullptr) {
  EdgeGeom g{};
  g.ctr_pts = pts_in, g.ctr_frames = frames_in, g.nb_pts = pts_out, g.nb_frames = frames_out;
  g.nbr = t_samples, g.nbr_stride = 1, g.nbr_offset = 0, g.ends = t_ends;
  g.n_ctr = s->n_in, g.f_ctr = s->f_in, g.f_nb = s->f_out, g.transposed = 1;
  g.n_nb = s->n_out;
  g.n_edges = s->n_edges;
  return g;
}

// The geometry records of a call.  Where they live: the caller's buffers (se3conv_prepared) where it keeps them, the
// workspace slots otherwise; a cloud against itself has one set of records for both sides.  The records this call has to
// build become jobs of `pb`; the forward view `g` and, in backward, the transposed view `gt` get their pointers.
void prepare_geometry(PrepBatch& pb, const se3conv_prepared* prep, const se3conv_shape* s, float* ws_in, float* ws_out,
                      EdgeGeom* g, EdgeGeom* gt) {
  const float *pts_in = g->nb_pts, *frames_in = g->nb_frames, *pts_out = g->ctr_pts, *frames_out = g->ctr_frames;
  const bool same_cloud = pts_in == pts_out && frames_in == frames_out && s->n_in == s->n_out && s->f_in == s->f_out;
  float *in = ws_in, *out = ws_out;
  bool need_in = true, need_out = true;
  if (prep && prep->geom_in) in = prep->geom_in, need_in = !prep->geom_in_valid;
  if (same_cloud) out = in, need_out = false;
  else if (prep && prep->geom_out) out = prep->geom_out, need_out = !prep->geom_out_valid;
  if (need_in) pb.geometry(pts_in, frames_in, s->n_in, s->f_in, in);
  if (need_out) pb.geometry(pts_out, frames_out, s->n_out, s->f_out, out);
  g->ctr_geom = out, g->nb_geom = in;
  if (gt) gt->ctr_geom = in, gt->nb_geom = out;
}

// Format of the row-sized intermediates (T, and U of the feature gradient): 0 packed hi|lo words (4 bytes per element), 1
// the 3-byte rows of common.h when the edge kernel can produce them (edge_t_bf16_t24_rows) and the buffer-load GEMMs consume
// them (SE3_NO_T24=1: packed words everywhere), 2 the 2.25-byte block format T16 -- only in SE3_PRECISION_BF16X3_T16, where
// the wave-pair edge kernel produces it (rows of a multiple of 64 channels); other shapes of that mode fall back to 1 / 0.
// tn_cols = the column count of the TN product that also reads the rows (0: none).  Any row count: the GEMMs that read the
// rows walk them in blocks their 32-bit offsets reach (gemm_bf16.hip).
int row_format(const se3conv_shape* s, const EdgeGeom& g, int channels, int tn_cols) {
  const bool on = !switches().no_t24;
  if (s->precision == SE3_PRECISION_BF16X3_T16 && kBasis == 32 && edge_t_bf16_t16_rows(g, channels) && tn_cols % 4 == 0)
    return 2;
  return on && kBasis == 32 && channels % 2 == 0 && edge_t_bf16_t24_rows(g, channels) && tn_cols % 4 == 0 ? 1 : 0;
}
// T: written by the forward pass, read by its GEMM and by the weight gradient's TN product (both plans)
int t_row_format(const se3conv_shape* s) { return row_format(s, forward_geom(s), s->c_in, s->c_out); }

// ---- the plans of a K = 32 call -------------------------------------------------------------------------------------
// Everything that is decided about HOW a call runs, and where its tensors live in the workspace, is decided here, once,
// from the shape and the request: the workspace queries, se3conv_bwd_needs_t, the traffic queries and the calls
// themselves read the same struct.  (Other K: the wrappers plan their inner K = 32 calls, see slice_params_kernel.)

struct FwdPlan {
  int fmt_t;  // row format of T (row_format)
  size_t axes_ext, t, featpk, bt_hi, bt_lo, split, geom_in, geom_out, total;
};
FwdPlan plan_fwd(const se3conv_shape* s, bool save_t) {
  FwdPlan p{};
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  const size_t kb = s->num_basis;
  const bool fast = s->precision != SE3_PRECISION_FP32;
  p.fmt_t = fast ? t_row_format(s) : 0;
  p.axes_ext = take(kDescExt * kBasis * 4);
  p.t = save_t ? 0 : take((size_t)s->n_out * s->f_out * s->c_in * kb * 4);
  if (fast) {
    p.featpk = take((size_t)s->n_in * s->f_in * s->c_in * 4);
    const size_t plane = (size_t)s->c_out * align_up((size_t)s->c_in * kb, 32) * 2;
    p.bt_hi = take(plane);
    p.bt_lo = take(plane);
    p.split = take(gemm_nn_bf16_split_bytes((int64_t)s->n_out * s->f_out, s->c_out, s->c_in * (int)kb));
  } else {
    p.split = take(gemm_nn_split_bytes((int64_t)s->n_out * s->f_out, s->c_out, s->c_in * (int)kb));
  }
  p.geom_in = take((size_t)s->n_in * s->f_in * 64);
  p.geom_out = take((size_t)s->n_out * s->f_out * 64);
  p.total = off;
  return p;
}

enum class FeatGrad { none, u, edge_major };               // the feature gradient: U rows + the grad_X GEMM, or edge_dx.hip
enum class WeightGrad { none, t_saved, t_recomputed, u };  // the tensor the weight gradient's product reads

// How a backward call runs.  Made from the shape and from WHAT is asked for -- a feature gradient, any parameter gradient,
// with or without a saved T -- not from which of grad_axes / grad_biases / grad_weights the call passes: a NULL pointer
// among them only skips the stage that would write it, it never selects another buffer or another form.
struct BwdPlan {
  bool fast;           // split-bf16 arithmetic (exact fp32 otherwise)
  bool feat_branch;    // the feature gradient has rows to run on: want_feat && rows_in > 0.  (The form, and what is reserved
                       // for it, follow the request alone: a U form on zero rows reserves its weight planes and launches nothing.)
  FeatGrad feat;
  WeightGrad dw;
  bool grad_t;         // grad_T is computed: for the parameter gradients, and as the operand of the edge-major form ...
  bool strip_t;        // ... by the row-strip GEMM (else the tiled one); the weights are prepared in its fragment layout
  int fmt_t, fmt_u;    // row formats of T and of U (row_format)
  bool share_dense;    // the dense products (grad_T, grad_X, the weight gradient's) run as roles of one launch: plan_dense_shared
  struct { int64_t m; int ka, n, splits; } tn;  // the weight gradient's TN product: over the rows of U or over those of T
  int n_param_partials;
  // Workspace offsets.  `big`: grad_T, and U when grad_T is not there at the same time.  `u`, `split_x`: where U and the
  // split-K partials of the grad_X GEMM go -- slots of their own when both branches run, `big` and `split` otherwise.
  // `bx_*`: the weight planes of the grad_X GEMM.  `dx_rows`: D [edge rows * F_in, C_in] fp32 of the edge-major form.
  size_t axes_ext, wt, w2, bt_hi, bt_lo, featpk, gpk, split, geom_in, geom_out, big, bx_hi, bx_lo, u, split_x, dx_rows, t,
      param_partials, tn_partials, total;
};
// The feature gradient of a convolution with many more input rows than edges per row can carry (a down-convolution)
// goes edge-major (edge_dx.hip): D = phi gT^T per frame-edge, summed per source row -- instead of a U row per source
// row and its GEMM.  Decided from the shape alone, for plan_bwd when a feature gradient is wanted: implemented shapes only,
// split-bf16 arithmetic, and the bytes the two forms move through memory -- U written and read (3-byte rows) against D written
// and gathered, plus grad_T when the parameter gradients do not need it anyway -- with a factor of two in favour of the
// default.  SE3_DX_PATH=0 never, =1 whenever implemented (tests force both on the same shapes).
bool plan_edge_major(const se3conv_shape* s, bool want_params) {
  const int mode = switches().dx_path;
  if (mode == 0 || s->precision == SE3_PRECISION_FP32) return false;
  if (s->n_in == 0 || s->n_out == 0) return false;
  if (!edge_dx_bf16_applicable(forward_geom(s), s->c_in)) return false;
  if (s->n_edges * s->f_in * (int64_t)s->c_in >= (1ll << 31)) return false;
  if (mode == 1) return true;
  const double rows_in = (double)s->n_in * s->f_in, rows_out = (double)s->n_out * s->f_out;
  const double u_bytes = rows_in * s->c_out * kBasis * 6.0;
  const double d_bytes = (double)s->n_edges * s->f_in * s->c_in * 8.0 + (want_params ? 0.0 : rows_out * s->c_in * kBasis * 8.0);
  // Cost model in microseconds, fitted in round 5 to the stage times of the reference network's own convolution calls
  // (profiles/r05_faust_network_convs.txt: the default against SE3_DX_PATH=1) and of the bench levels: the U form pays a
  // latency floor for its two launches on levels too small to fill the chip (~45 us: the grad_X GEMM of a 3.7 k-row level
  // takes as long as that of an 18 k-row one) plus its bytes at the rate of a just-written tensor; the edge-major form
  // ~15 us plus its bytes at the rate of its row gathers -- and loses whatever the bytes say where a source owns more than
  // ~20 edges (its per-source sum walks the segment: headline level 2, 27 edges per point, 0.108 -> 0.115 ms; a lateral
  // convolution with 357 edges per source: dx_gather 330 us).  Round 4's rule was 2 d_bytes < u_bytes.
  if ((double)s->n_edges > 20.0 * (double)s->n_in) return false;
  return 15.0 + d_bytes / 2.2e6 < 45.0 + u_bytes / 6.0e6;
}

// Whether the dense products of a backward call share a launch (gemm_bf16.hip, bwd_dense_shared_kernel).  On a level that
// does not fill the chip the products are launches one after the other on a machine none of them fills; as roles of one
// grid they run side by side and the level saves a launch per role.  Decided from the shape and the request: split-bf16
// arithmetic; a level of at most Switches::dense_share_rows rows on either side (the gate: profiles/bwd_dense_shared.txt;
// SE3_DX_PATH=-1,dense=0 forces separate launches); every product the request can run is one the shared kernel has a body for
// (the buffer-load forms over packed words and 3-byte rows -- not the T16 rows, not the guarded-load forms); at least two
// products.  A call that passes no grad_weights runs one product fewer: with one left it launches that one as ever.
bool plan_dense_shared(const se3conv_shape* s, const BwdPlan& p, bool want_params) {
  const int64_t rows_out = s->n_out * s->f_out, rows_in = s->n_in * s->f_in, gate = switches().dense_share_rows;
  if (!p.fast || rows_in <= 0 || rows_out <= 0 || rows_in > gate || rows_out > gate) return false;
  const int ck = s->c_in * s->num_basis, cok = s->c_out * s->num_basis;
  const bool x_role = p.feat_branch && p.feat == FeatGrad::u;
  if ((int)p.grad_t + (int)x_role + (int)want_params < 2) return false;
  if (p.grad_t && !p.strip_t && !gemm_nn_bf16_sharable(rows_out, ck, s->c_out, true, 0)) return false;
  if (x_role && !gemm_nn_bf16_sharable(rows_in, s->c_in, cok, false, p.fmt_u)) return false;
  if (want_params && !gemm_tn_bf16_sharable(p.tn.m, p.tn.ka, p.tn.n, p.tn.splits, p.dw == WeightGrad::u ? p.fmt_u : p.fmt_t)) return false;
  return true;
}

BwdPlan plan_bwd(const se3conv_shape* s, bool want_feat, bool want_params, bool have_t) {
  BwdPlan p{};
  const size_t kb = s->num_basis;
  const size_t rows_out = (size_t)s->n_out * s->f_out, rows_in = (size_t)s->n_in * s->f_in;
  const int ck = s->c_in * (int)kb, cok = s->c_out * (int)kb;
  p.fast = s->precision != SE3_PRECISION_FP32;
  p.feat_branch = want_feat && rows_in > 0;
  p.feat = !want_feat ? FeatGrad::none : plan_edge_major(s, want_params) ? FeatGrad::edge_major : FeatGrad::u;
  const bool u_form = p.feat == FeatGrad::u, edge_major = p.feat == FeatGrad::edge_major;
  p.grad_t = want_params || edge_major;
  if (p.fast) {
    p.strip_t = gemm_strip_bf16_applicable((int64_t)rows_out, ck, s->c_out);  // grad_T = g W^T
    p.fmt_t = t_row_format(s);
    p.fmt_u = row_format(s, transposed_geom(s), s->c_out, 0);
  }
  // The weight gradient from U instead of T (round 5): dW[i,k,o] = alpha sum_p f[p,i] U[p,o,k] -- U is the transposed pass's
  // tensor, which backward produces anyway for the feature gradient.  Available in the split-bf16 modes whenever the U form
  // of the feature gradient runs; then the forward pass need not keep T (0.8 GB per layer at the headline shape: the largest
  // saved activation by a factor of 24), and for an up-convolution the product walks the few rows of the coarse level
  // instead of the many of the fine one.  Used when T was not saved, or when U has fewer (row x channel) entries than T.
  const bool dw_u = p.fast && u_form && p.feat_branch && want_params && rows_out > 0 && s->c_in % 4 == 0 && s->c_out % 2 == 0 &&
                    (!have_t || (double)rows_in * s->c_out < (double)rows_out * s->c_in);
  p.dw = !want_params ? WeightGrad::none : dw_u ? WeightGrad::u : have_t ? WeightGrad::t_saved : WeightGrad::t_recomputed;
  if (dw_u) p.tn = {(int64_t)rows_in, cok, s->c_in, 0};
  else p.tn = {(int64_t)rows_out, ck, s->c_out, 0};
  p.tn.splits = gemm_tn_splits(p.tn.m, p.tn.ka, p.tn.n);
  p.n_param_partials = edge_param_grad_blocks((int64_t)rows_out);
  p.share_dense = plan_dense_shared(s, p, want_params);

  // The workspace.  Callers cache these sizes: a reservation that is wider than its use (the packed feature words although
  // the caller may bring them, se3conv_prepared; the grad_X planes of a U form on zero rows) stays as wide.
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  const size_t wsz = (size_t)s->c_in * kb * s->c_out * 4;
  const size_t t_bytes = rows_out * s->c_in * kb * 4, u_bytes = rows_in * s->c_out * kb * 4;  // grad_T and a recomputed T; U
  p.axes_ext = take(kDescExt * kBasis * 4);
  if (!p.fast) {
    p.wt = want_params ? take(wsz) : 0;
    p.w2 = u_form ? take(wsz) : 0;
    p.split = u_form ? take(gemm_nn_split_bytes((int64_t)rows_in, s->c_in, cok)) : 0;
  } else {
    // the largest of the three pre-split weight layouts (see prep_weights_kernel)
    size_t plane = (size_t)s->c_in * kb * align_up((size_t)s->c_out, 32) * 2;
    const size_t p2 = (size_t)s->c_in * align_up((size_t)s->c_out * kb, 32) * 2;
    if (p2 > plane) plane = p2;
    const size_t p3 = (size_t)s->c_out * kb * align_up((size_t)s->c_in, 32) * 2;
    if (p3 > plane) plane = p3;
    p.bt_hi = take(plane);
    p.bt_lo = take(plane);
    p.featpk = want_params ? take(rows_in * s->c_in * 4) : 0;
    p.gpk = take(rows_out * s->c_out * 4);
    size_t sp = p.grad_t ? gemm_nn_bf16_split_bytes((int64_t)rows_out, ck, s->c_out) : 0;
    const size_t sp3 = want_params ? gemm_nn_bf16_split_bytes((int64_t)rows_in, cok, s->c_in) : 0;
    if (sp3 > sp) sp = sp3;
    const size_t sp2 = u_form ? gemm_nn_bf16_split_bytes((int64_t)rows_in, s->c_in, cok) : 0;
    if (sp2 > sp) sp = sp2;
    p.split = take(sp);
  }
  p.geom_in = take(rows_in * 64);
  p.geom_out = take(rows_out * 64);
  // (the edge-major feature gradient has no U: none of the U-sized terms is reserved on that path -- at a down-convolution
  // of the headline hierarchy they were 2 GB of workspace nobody touched)
  size_t big = p.grad_t ? t_bytes : 0;
  if (u_form && u_bytes > big) big = u_bytes;
  p.big = take(big);
  if (p.fast && u_form) {
    const size_t p2 = (size_t)s->c_in * align_up((size_t)s->c_out * kb, 32) * 2;
    p.bx_hi = take(p2);
    p.bx_lo = take(p2);
  }
  const bool both = p.fast && u_form && want_params;  // both branches run: grad_T takes `big` while U is alive
  p.u = both ? take(u_bytes) : p.big;
  p.split_x = both ? take(gemm_nn_bf16_split_bytes((int64_t)rows_in, s->c_in, cok)) : p.split;
  p.dx_rows = edge_major ? take((size_t)s->n_edges * s->f_in * s->c_in * 4) : 0;
  p.t = p.dw == WeightGrad::t_recomputed ? take(t_bytes) : 0;
  p.param_partials = want_params ? take((size_t)p.n_param_partials * edge_param_grad_bf16_channel_blocks(s->c_in) *
                                         kDescExt * kBasis * 4) : 0;
  p.tn_partials = want_params ? take((size_t)p.tn.splits * wsz) : 0;
  p.total = off;
  return p;
}

// ---- any number of basis functions on the K = 32 kernels (se3conv_fwd / se3conv_bwd with num_basis != 32) ---------------
// The sum over k is separable: K basis functions are ceil(K / 32) slices of 32, the last one padded with basis functions
// whose projection axes, bias and conv weights are zero (GELU(0) = 0 meets W = 0: exact).  Per slice the padded parameter
// copies are built in the workspace, the K = 32 operator runs on them, outputs are accumulated and the parameter gradients
// copied back into their slice of the caller's tensors.  T is not kept between the calls for K != 32 (`t_save` ignored).
__global__ void slice_params_kernel(const float* __restrict__ axes, const float* __restrict__ biases,
                                    const float* __restrict__ w, int kb, int k0, int kn, int c_in, int c_out,
                                    float* __restrict__ a32, float* __restrict__ b32, float* __restrict__ w32) {
  const int64_t n_w = (int64_t)c_in * kBasis * c_out;
  // the axes / bias tables (288 + 32 entries) ride in the same loop: it runs to whichever is longer (c_in * c_out < 9)
  const int64_t n_all = n_w > SE3_DESC_DIMS * kBasis ? n_w : SE3_DESC_DIMS * kBasis;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(i % c_out);
    const int k = (int)((i / c_out) % kBasis);
    const int ci = (int)(i / ((int64_t)c_out * kBasis));
    if (i < n_w) w32[i] = k < kn ? w[((int64_t)ci * kb + k0 + k) * c_out + o] : 0.f;
    if (i < SE3_DESC_DIMS * kBasis) {
      const int j = (int)(i / kBasis), kk = (int)(i % kBasis);
      a32[i] = kk < kn ? axes[j * kb + k0 + kk] : 0.f;
    }
    if (i < kBasis) b32[i] = i < kn ? biases[k0 + i] : 0.f;
  }
}

__global__ void unslice_grads_kernel(const float* __restrict__ da32, const float* __restrict__ db32,
                                     const float* __restrict__ dw32, int kb, int k0, int kn, int c_in, int c_out,
                                     float* __restrict__ grad_axes, float* __restrict__ grad_biases,
                                     float* __restrict__ grad_weights) {
  const int64_t n_w = (int64_t)c_in * kBasis * c_out;
  const int64_t n_all = n_w > SE3_DESC_DIMS * kBasis ? n_w : SE3_DESC_DIMS * kBasis;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(i % c_out);
    const int k = (int)((i / c_out) % kBasis);
    const int ci = (int)(i / ((int64_t)c_out * kBasis));
    if (grad_weights && i < n_w && k < kn) grad_weights[((int64_t)ci * kb + k0 + k) * c_out + o] = dw32[i];
    if (grad_axes && i < SE3_DESC_DIMS * kBasis) {
      const int j = (int)(i / kBasis), kk = (int)(i % kBasis);
      if (kk < kn) grad_axes[j * kb + k0 + kk] = da32[i];
    }
    if (grad_biases && i < kn) grad_biases[k0 + i] = db32[i];
  }
}

__global__ void add_into_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

struct AnyBasisLayout { size_t a32, b32, w32, out_tmp, da32, db32, dw32, inner, total; int slices; };
AnyBasisLayout any_basis_layout(const se3conv_shape* s, size_t out_tmp_bytes, bool grads, size_t inner_bytes) {
  AnyBasisLayout l{};
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
  const size_t wsz = (size_t)s->c_in * kBasis * s->c_out * 4;
  l.slices = (s->num_basis + kBasis - 1) / kBasis;
  l.a32 = take(SE3_DESC_DIMS * kBasis * 4);
  l.b32 = take(kBasis * 4);
  l.w32 = take(wsz);
  l.out_tmp = take(l.slices > 1 ? out_tmp_bytes : 0);
  if (grads) {
    l.da32 = take(SE3_DESC_DIMS * kBasis * 4);
    l.db32 = take(kBasis * 4);
    l.dw32 = take(wsz);
  }
  l.inner = take(inner_bytes);
  l.total = off;
  return l;
}
// work items of slice_params_kernel / unslice_grads_kernel: the weights or the 288-entry axes table, whichever is longer
int64_t slice_items(const se3conv_shape* s) {
  const int64_t n_w = (int64_t)s->c_in * kBasis * s->c_out;
  return n_w > SE3_DESC_DIMS * kBasis ? n_w : SE3_DESC_DIMS * kBasis;
}
se3conv_shape with_32_basis(const se3conv_shape* s) {
  se3conv_shape t = *s;
  t.num_basis = kBasis;
  return t;
}

}  // namespace
}  // namespace se3

using namespace se3;

extern "C" int se3_abi_version(void) { return SE3_ABI_VERSION; }

extern "C" const char* se3_error_string(int code) {
  switch (code) {
    case SE3_OK: return "ok";
    case SE3_ERR_INVALID_ARGUMENT: return "invalid argument (null pointer, negative size or bad shape)";
    case SE3_ERR_UNSUPPORTED: return "unsupported shape (int32-sized clouds; API-parity ops: K in {8, 16, 32, 64})";
    case SE3_ERR_WORKSPACE: return "workspace too small";
    case SE3_ERR_LAUNCH: return "HIP launch/runtime error";
    default: return "unknown error";
  }
}

extern "C" int se3_rot_tensors_rel(const float* pts_in, const float* pts_out, const float* frames_in,
                                   const float* frames_out, const int32_t* neighbors, const int32_t* ends,
                                   const float* rho, const se3conv_shape* s, int32_t rel_rot, float* desc,
                                   int32_t* fe_neighbors, int32_t* fe_ends, void* stream_) {
  if (!shape_ok(s) || rel_rot < SE3_REL_ROT_6D || rel_rot > SE3_REL_ROT_QUATERNION) return SE3_ERR_INVALID_ARGUMENT;
  if (s->n_edges * s->f_in * s->f_out >= (1ll << 31)) return SE3_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  if (s->n_out > 0) {
    if (!ends || !fe_ends) return SE3_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(rot_tensor_ends_kernel, dim3(grid_for(s->n_out * s->f_out)), dim3(256), 0, stream, ends, s->n_out,
                       s->f_in, s->f_out, fe_ends);
  }
  if (s->n_edges > 0) {
    if (!pts_in || !pts_out || !frames_in || !frames_out || !neighbors || !ends || !rho || !desc || !fe_neighbors)
      return SE3_ERR_INVALID_ARGUMENT;
    const dim3 grid(grid_for(s->n_edges * s->f_in * s->f_out));
#define SE3_ROT(REL)                                                                                                  \
  hipLaunchKernelGGL(rot_tensors_kernel<REL>, grid, dim3(256), 0, stream, pts_in, pts_out, frames_in, frames_out, neighbors, \
                     ends, rho, s->n_edges, s->f_in, s->f_out, desc, fe_neighbors)
    if (rel_rot == SE3_REL_ROT_6D) SE3_ROT(0);
    else if (rel_rot == SE3_REL_ROT_MATRIX) SE3_ROT(1);
    else SE3_ROT(2);
#undef SE3_ROT
  }
  return check_launch();
}

extern "C" int se3_rot_tensors(const float* pts_in, const float* pts_out, const float* frames_in,
                               const float* frames_out, const int32_t* neighbors, const int32_t* ends,
                               const float* rho, const se3conv_shape* s, float* desc, int32_t* fe_neighbors,
                               int32_t* fe_ends, void* stream) {
  return se3_rot_tensors_rel(pts_in, pts_out, frames_in, frames_out, neighbors, ends, rho, s, SE3_REL_ROT_6D, desc,
                             fe_neighbors, fe_ends, stream);
}

static bool basis_count_ok(int kb) { return kb == 8 || kb == 16 || kb == 32 || kb == 64; }

extern "C" int se3_feat_basis_proj(const float* basis, const float* feat, const int32_t* neighbors, const int32_t* ends,
                                   int64_t n_edges, int64_t n_rows, int64_t n_feat, int32_t channels,
                                   int32_t num_basis, float* out, void* stream) {
  if (n_edges < 0 || n_rows < 0 || n_feat < 0 || channels < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (!basis_count_ok(num_basis)) return SE3_ERR_UNSUPPORTED;  // feat_basis_utils.cuh:35-41
  if (n_rows == 0) return SE3_OK;
  if (!ends || !out || (n_edges > 0 && (!basis || !feat || !neighbors))) return SE3_ERR_INVALID_ARGUMENT;
  if (n_rows >= (1ll << 31)) return SE3_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(feat_basis_proj_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, basis, feat,
                     neighbors, ends, channels, num_basis, out);
  return check_launch();
}

extern "C" int se3_feat_basis_proj_grad(const float* basis, const float* feat, const int32_t* neighbors,
                                        const int32_t* ends, const float* grad_out, int64_t n_edges, int64_t n_rows,
                                        int64_t n_feat, int32_t channels, int32_t num_basis, float* g_feat,
                                        float* g_basis, void* stream_) {
  if (n_edges < 0 || n_rows < 0 || n_feat < 0 || channels < 1) return SE3_ERR_INVALID_ARGUMENT;
  if (!basis_count_ok(num_basis)) return SE3_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  if (n_feat > 0) {
    if (!g_feat) return SE3_ERR_INVALID_ARGUMENT;
    if (int rc = launch_fill_words(g_feat, 0u, n_feat * channels, stream)) return rc;
  }
  if (n_edges == 0) return SE3_OK;
  if (!basis || !feat || !neighbors || !ends || !grad_out || !g_basis) return SE3_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(feat_basis_proj_grad_basis_kernel, dim3(grid_for(n_edges * num_basis)), dim3(256), 0, stream, feat,
                     neighbors, ends, grad_out, n_edges, n_rows, channels, num_basis, g_basis);
  hipLaunchKernelGGL(feat_basis_proj_grad_feat_kernel, dim3(grid_for(n_edges * channels)), dim3(256), 0, stream, basis,
                     neighbors, ends, grad_out, n_edges, n_rows, channels, num_basis, g_feat);
  return check_launch();
}

// Bytes per element of the row-sized intermediates this shape would move (what a traffic model has to assume):
// which = 0: T (forward, read again by the weight gradient), 1: U (feature gradient), 2: grad_T.  < 0: bad shape.
// The T16 format's 2.25 bytes are reported as 2 here (an integer interface); se3conv_intermediate_row_bytes is exact.
static int64_t intermediate_row_bytes(const se3conv_shape* s, int which) {
  const int64_t ck = (int64_t)(which == 1 ? s->c_out : s->c_in) * s->num_basis;
  if (s->precision == SE3_PRECISION_FP32 || s->num_basis != kBasis || which == 2) return ck * 4;  // (grad_T: packed words)
  const BwdPlan p = plan_bwd(s, true, true, false);
  const int fmt = which == 0 ? p.fmt_t : p.fmt_u;
  return fmt == 2 ? t16_row_bytes(which == 0 ? s->c_in : s->c_out) : ck * (fmt == 1 ? 3 : 4);
}
extern "C" int64_t se3conv_intermediate_row_bytes(const se3conv_shape* s, int which) {
  if (!shape_ok(s) || which < 0 || which > 2) return SE3_ERR_INVALID_ARGUMENT;
  return intermediate_row_bytes(s, which);
}
extern "C" int se3conv_intermediate_bytes_per_element(const se3conv_shape* s, int which) {
  if (!shape_ok(s) || which < 0 || which > 2) return SE3_ERR_INVALID_ARGUMENT;
  const int64_t ck = (int64_t)(which == 1 ? s->c_out : s->c_in) * s->num_basis;
  return (int)(intermediate_row_bytes(s, which) / ck);
}

extern "C" size_t se3conv_fwd_workspace_bytes(const se3conv_shape* s, int save_t) {
  if (!shape_ok(s)) return 0;
  if (s->num_basis != kBasis) {
    const se3conv_shape s32 = with_32_basis(s);
    return any_basis_layout(s, (size_t)s->n_out * s->f_out * s->c_out * 4, false, plan_fwd(&s32, false).total).total;
  }
  return plan_fwd(s, save_t != 0).total;
}

extern "C" int se3conv_fwd(const float* pts_in, const float* pts_out, const float* frames_in, const float* frames_out,
                           const int32_t* neighbors, const int32_t* ends, const float* feat, const float* proj_axes,
                           const float* proj_biases, const float* conv_weights, const float* rho, const float* nu,
                           const se3conv_shape* s, float* out, float* t_save, void* workspace, size_t workspace_bytes,
                           void* stream_) {
  return se3conv_fwd_prepared(pts_in, pts_out, frames_in, frames_out, neighbors, ends, feat, proj_axes, proj_biases, conv_weights,
                              rho, nu, s, out, t_save, workspace, workspace_bytes, stream_, nullptr);
}

// NOTE for whoever adds a device call to se3conv_fwd_prepared / se3conv_bwd_prepared or to a launcher below them: the
// se3conv_forms query (end of this file) runs these very functions with dummy pointers while forms_only() is true.  Every
// launch, event, memset or runtime query on that path must sit behind `if (!forms_only())` (or inside a launcher, after its
// form_report); pointers derived from the workspace may be computed but never dereferenced on the host.
extern "C" int se3conv_fwd_prepared(const float* pts_in, const float* pts_out, const float* frames_in, const float* frames_out,
                                    const int32_t* neighbors, const int32_t* ends, const float* feat, const float* proj_axes,
                                    const float* proj_biases, const float* conv_weights, const float* rho, const float* nu,
                                    const se3conv_shape* s, float* out, float* t_save, void* workspace, size_t workspace_bytes,
                                    void* stream_, const se3conv_prepared* prep) {
  if (!shape_ok(s)) return SE3_ERR_INVALID_ARGUMENT;
  if (s->num_basis != kBasis) {
    // slices of 32 basis functions on the K = 32 operator (see slice_params_kernel); t_save is not written
    if (s->n_out == 0) return SE3_OK;
    if (!proj_axes || !proj_biases || !conv_weights || !out || !workspace) return SE3_ERR_INVALID_ARGUMENT;
    const se3conv_shape s32 = with_32_basis(s);
    const int64_t n_out_el = s->n_out * s->f_out * s->c_out;
    const AnyBasisLayout l = any_basis_layout(s, (size_t)n_out_el * 4, false, plan_fwd(&s32, false).total);
    if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float *a32 = (float*)(ws + l.a32), *b32 = (float*)(ws + l.b32), *w32 = (float*)(ws + l.w32);
    for (int sl = 0; sl < l.slices; ++sl) {
      const int k0 = sl * kBasis, kn = s->num_basis - k0 < kBasis ? s->num_basis - k0 : kBasis;
      if (!forms_only())
        hipLaunchKernelGGL(slice_params_kernel, dim3(grid_for(slice_items(s))), dim3(256), 0, stream,
                           proj_axes, proj_biases, conv_weights, s->num_basis, k0, kn, s->c_in, s->c_out, a32, b32, w32);
      float* dst = sl == 0 ? out : (float*)(ws + l.out_tmp);
      if (int rc = se3conv_fwd(pts_in, pts_out, frames_in, frames_out, neighbors, ends, feat, a32, b32, w32, rho, nu, &s32, dst,
                               nullptr, ws + l.inner, l.total - l.inner, stream_))
        return rc;
      if (sl > 0 && !forms_only())
        hipLaunchKernelGGL(add_into_kernel, dim3(grid_for(n_out_el)), dim3(256), 0, stream, out, dst, n_out_el);
    }
    return check_launch();
  }
  if (int rc = shape_supported(s)) return rc;
  if (s->n_out == 0) return SE3_OK;
  if (!pts_out || !frames_out || !ends || !proj_axes || !proj_biases || !conv_weights || !rho || !nu || !out ||
      !workspace || (s->n_edges > 0 && (!pts_in || !frames_in || !neighbors || !feat)))
    return SE3_ERR_INVALID_ARGUMENT;
  const FwdPlan p = plan_fwd(s, t_save != nullptr);
  if (workspace_bytes < p.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  float* axes_ext = (float*)(ws + p.axes_ext);
  float* t = t_save ? t_save : (float*)(ws + p.t);

  EdgeGeom g = forward_geom(s, pts_in, pts_out, frames_in, frames_out, neighbors, ends);
  const int64_t rows_out = s->n_out * s->f_out;
  const int ck = s->c_in * s->num_basis;
  const float inv_fin = 1.0f / (float)s->f_in;
  // einsum('nik,iko->no') :210, /F_in :213, *norm_num_neighs_ :216 are the GEMM + its alpha
  PrepBatch pb;  // one launch: [A; beta] table, packed geometry records; split-bf16: packed feature words, weight planes
  pb.axes(proj_axes, proj_biases, axes_ext);
  prepare_geometry(pb, prep, s, (float*)(ws + p.geom_in), (float*)(ws + p.geom_out), &g, nullptr);
  if (s->precision == SE3_PRECISION_FP32) {
    if (int rc = pb.launch(stream)) return rc;
    if (int rc = launch_edge_t("edge_t_fwd", g, feat, s->c_in, s->n_in * s->f_in, axes_ext, rho, t, stream)) return rc;
    return launch_gemm_nn("gemm_out", t, conv_weights, out, rows_out, s->c_out, ck, nu, inv_fin, stream, (float*)(ws + p.split));
  }
  // (packed feature words: into the caller's buffer where backward will want them again)
  uint32_t* featpk = prep && prep->feat_words ? prep->feat_words : (uint32_t*)(ws + p.featpk);
  const bool need_featpk = !(prep && prep->feat_words && prep->feat_words_valid);
  uint16_t* bt_hi = (uint16_t*)(ws + p.bt_hi);
  uint16_t* bt_lo = (uint16_t*)(ws + p.bt_lo);
  const float inv_phi = inv_fin / kGeluOut;  // the bf16 edge kernels produce kGeluOut * phi (gelu_scaled)
  if (need_featpk) pb.split(feat, featpk, s->n_in * s->f_in * s->c_in);
  pb.weights(conv_weights, s->c_in, s->num_basis, s->c_out, 0, bt_hi, bt_lo, nullptr, 1.0f, false, p.fmt_t);
  if (int rc = pb.launch(stream)) return rc;
  if (int rc = launch_edge_t_bf16("edge_t_fwd", g, featpk, s->c_in, s->n_in * s->f_in, axes_ext, rho, (uint32_t*)t, stream, p.fmt_t))
    return rc;
  return launch_gemm_nn_bf16("gemm_out", (const uint32_t*)t, bt_hi, bt_lo, out, false, rows_out, s->c_out, ck,
                             (float*)(ws + p.split), nu, inv_phi, stream, p.fmt_t);
}

extern "C" int se3conv_bwd_needs_t(const se3conv_shape* s, int want_feat) {
  if (!shape_ok(s)) return SE3_ERR_INVALID_ARGUMENT;
  if (s->num_basis != kBasis) return 0;  // other K: T is recomputed per slice of 32 basis functions, `t_save` is never read
  return plan_bwd(s, want_feat != 0, true, false).dw == WeightGrad::u ? 0 : 1;
}

extern "C" size_t se3conv_bwd_workspace_bytes(const se3conv_shape* s, int want_feat, int want_params, int have_t) {
  if (!shape_ok(s)) return 0;
  if (s->num_basis != kBasis) {
    const se3conv_shape s32 = with_32_basis(s);
    return any_basis_layout(s, want_feat ? (size_t)s->n_in * s->f_in * s->c_in * 4 : 0, want_params != 0,
                            plan_bwd(&s32, want_feat != 0, want_params != 0, false).total).total;
  }
  return plan_bwd(s, want_feat != 0, want_params != 0, have_t != 0).total;
}

extern "C" int se3conv_bwd(const float* pts_in, const float* pts_out, const float* frames_in, const float* frames_out,
                           const int32_t* neighbors, const int32_t* ends, const int32_t* t_samples,
                           const int32_t* t_ends, const int32_t* t_edge_ids, const float* feat, const float* proj_axes,
                           const float* proj_biases,
                           const float* conv_weights, const float* rho, const float* nu, const float* t_save,
                           const float* grad_out, const se3conv_shape* s, float* grad_feat, float* grad_axes,
                           float* grad_biases, float* grad_weights, void* workspace, size_t workspace_bytes,
                           void* stream_) {
  return se3conv_bwd_prepared(pts_in, pts_out, frames_in, frames_out, neighbors, ends, t_samples, t_ends, t_edge_ids, feat, proj_axes,
                              proj_biases, conv_weights, rho, nu, t_save, grad_out, s, grad_feat, grad_axes, grad_biases, grad_weights,
                              workspace, workspace_bytes, stream_, nullptr);
}

extern "C" int se3conv_bwd_prepared(const float* pts_in, const float* pts_out, const float* frames_in, const float* frames_out,
                                    const int32_t* neighbors, const int32_t* ends, const int32_t* t_samples,
                                    const int32_t* t_ends, const int32_t* t_edge_ids, const float* feat, const float* proj_axes,
                                    const float* proj_biases, const float* conv_weights, const float* rho, const float* nu,
                                    const float* t_save, const float* grad_out, const se3conv_shape* s, float* grad_feat,
                                    float* grad_axes, float* grad_biases, float* grad_weights, void* workspace,
                                    size_t workspace_bytes, void* stream_, const se3conv_prepared* prep) {
  if (!shape_ok(s)) return SE3_ERR_INVALID_ARGUMENT;
  if (s->num_basis != kBasis) {
    // slices of 32 basis functions (see slice_params_kernel): T is recomputed per slice (t_save ignored), dX is the sum of
    // the slices' feature gradients, every slice writes its own columns of the parameter gradients
    const bool wf = grad_feat != nullptr, wp = grad_axes || grad_biases || grad_weights;
    if (!wf && !wp) return SE3_OK;
    if (!proj_axes || !proj_biases || !conv_weights || !workspace) return SE3_ERR_INVALID_ARGUMENT;
    const se3conv_shape s32 = with_32_basis(s);
    const int64_t n_in_el = s->n_in * s->f_in * s->c_in;
    const AnyBasisLayout l = any_basis_layout(s, wf ? (size_t)n_in_el * 4 : 0, wp, plan_bwd(&s32, wf, wp, false).total);
    if (workspace_bytes < l.total) return SE3_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float *a32 = (float*)(ws + l.a32), *b32 = (float*)(ws + l.b32), *w32 = (float*)(ws + l.w32);
    float *da32 = wp ? (float*)(ws + l.da32) : nullptr, *db32 = wp ? (float*)(ws + l.db32) : nullptr;
    float* dw32 = wp ? (float*)(ws + l.dw32) : nullptr;
    const dim3 pgrid(grid_for(slice_items(s)));
    for (int sl = 0; sl < l.slices; ++sl) {
      const int k0 = sl * kBasis, kn = s->num_basis - k0 < kBasis ? s->num_basis - k0 : kBasis;
      if (!forms_only())
        hipLaunchKernelGGL(slice_params_kernel, pgrid, dim3(256), 0, stream, proj_axes, proj_biases, conv_weights,
                           s->num_basis, k0, kn, s->c_in, s->c_out, a32, b32, w32);
      float* dx = !wf ? nullptr : (sl == 0 ? grad_feat : (float*)(ws + l.out_tmp));
      if (int rc = se3conv_bwd(pts_in, pts_out, frames_in, frames_out, neighbors, ends, t_samples, t_ends, t_edge_ids, feat, a32, b32, w32, rho,
                               nu, nullptr, grad_out, &s32, dx, da32, db32, dw32, ws + l.inner, l.total - l.inner, stream_))
        return rc;
      if (forms_only()) continue;
      if (wf && sl > 0 && n_in_el > 0)
        hipLaunchKernelGGL(add_into_kernel, dim3(grid_for(n_in_el)), dim3(256), 0, stream, grad_feat, dx, n_in_el);
      if (wp)
        hipLaunchKernelGGL(unslice_grads_kernel, pgrid, dim3(256), 0, stream, da32, db32, dw32, s->num_basis, k0, kn, s->c_in,
                           s->c_out, grad_axes, grad_biases, grad_weights);
    }
    return check_launch();
  }
  if (int rc = shape_supported(s)) return rc;
  const bool want_feat = grad_feat != nullptr;
  const bool want_params = grad_axes || grad_biases || grad_weights;
  if (!want_feat && !want_params) return SE3_OK;
  if (!proj_axes || !proj_biases || !conv_weights || !rho || !nu || !workspace) return SE3_ERR_INVALID_ARGUMENT;
  if (s->n_out > 0 && (!pts_out || !frames_out || !ends || !grad_out)) return SE3_ERR_INVALID_ARGUMENT;
  if (s->n_in > 0 && (!pts_in || !frames_in || !feat)) return SE3_ERR_INVALID_ARGUMENT;
  if (s->n_edges > 0 && !neighbors) return SE3_ERR_INVALID_ARGUMENT;
  if (want_feat && s->n_in > 0 && (!t_ends || (s->n_edges > 0 && !t_samples))) return SE3_ERR_INVALID_ARGUMENT;
  const BwdPlan p = plan_bwd(s, want_feat, want_params, t_save != nullptr);
  if (workspace_bytes < p.total) return SE3_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  float* axes_ext = (float*)(ws + p.axes_ext);
  float* big = (float*)(ws + p.big);
  const int kb = s->num_basis;
  const int ck = s->c_in * kb;
  const int64_t rows_out = s->n_out * s->f_out, rows_in = s->n_in * s->f_in;
  const float inv_fin = 1.0f / (float)s->f_in;
  float* partials = (float*)(ws + p.param_partials);
  float* tn_partials = (float*)(ws + p.tn_partials);

  EdgeGeom g = forward_geom(s, pts_in, pts_out, frames_in, frames_out, neighbors, ends);
  EdgeGeom gt = transposed_geom(s, pts_in, pts_out, frames_in, frames_out, t_samples, t_ends);
  // one launch: [A; beta] table and the packed geometry records of both sides; split-bf16: the packed words of g and f and
  // the weight planes too
  PrepBatch pb;
  pb.axes(proj_axes, proj_biases, axes_ext);
  prepare_geometry(pb, prep, s, (float*)(ws + p.geom_in), (float*)(ws + p.geom_out), &g, &gt);

  if (!p.fast) {
    if (int rc = pb.launch(stream)) return rc;
    if (want_params) {
      // gT[m,(i,k)] = alpha * sum_o g[m,o] W[i,k,o]
      float* wt = (float*)(ws + p.wt);
      if (!forms_only())
        hipLaunchKernelGGL(transpose_kernel, dim3(grid_for((int64_t)ck * s->c_out)), dim3(256), 0, stream, conv_weights,
                           wt, ck, s->c_out);
      if (int rc = launch_gemm_nn("gemm_gradT", grad_out, wt, big, rows_out, ck, s->c_out, nu, inv_fin, stream)) return rc;
      if (grad_axes || grad_biases) {
        int n_part = 0;
        if (int rc = launch_edge_param_grad("edge_param_grad", g, feat, s->c_in, rows_in, axes_ext, rho, big, partials,
                                            p.n_param_partials, &n_part, stream))
          return rc;
        if (!forms_only())
          hipLaunchKernelGGL(reduce_param_partials_kernel, dim3(kDescExt * kBasis), dim3(256), 0, stream, partials,
                             n_part, grad_axes, grad_biases, 1.0f);
      }
      if (grad_weights) {
        const float* t = t_save;
        if (p.dw == WeightGrad::t_recomputed) {
          float* tt = (float*)(ws + p.t);
          if (int rc = launch_edge_t("edge_t_recompute", g, feat, s->c_in, rows_in, axes_ext, rho, tt, stream)) return rc;
          t = tt;
        }
        // dW[(i,k),o] = alpha * sum_m T[m,(i,k)] g[m,o]
        if (int rc = launch_gemm_tn("gemm_gradW", t, grad_out, grad_weights, tn_partials, p.tn.splits, p.tn.m, p.tn.ka,
                                    p.tn.n, nu, inv_fin, stream))
          return rc;
      }
    }
    if (p.feat_branch) {
      // Transposed convolution instead of scatter atomics:
      //   U[(p,b),o,k] = sum_{edges into p} sum_a phi(s,a,p,b)[k] g[(s,a),o];  dX[(p,b),i] = alpha * sum_{o,k} U W[i,k,o]
      float* u = (float*)(ws + p.u);
      if (int rc = launch_edge_t("edge_t_transposed", gt, grad_out, s->c_out, rows_out, axes_ext, rho, u, stream)) return rc;
      float* w2 = (float*)(ws + p.w2);
      if (!forms_only())
        hipLaunchKernelGGL(permute_weights_oki_kernel, dim3(grid_for((int64_t)ck * s->c_out)), dim3(256), 0, stream,
                           conv_weights, w2, s->c_in, kb, s->c_out);
      if (int rc = launch_gemm_nn("gemm_gradX", u, w2, grad_feat, rows_in, s->c_in, s->c_out * kb, nu, inv_fin, stream,
                                  (float*)(ws + p.split_x)))
        return rc;
    }
    return check_launch();
  }

  // ---- split-bf16 path: same stages, operands as packed words -----------------------------------------
  const bool u_form = p.feat_branch && p.feat == FeatGrad::u, edge_major = p.feat == FeatGrad::edge_major;
  uint16_t* bt_hi = (uint16_t*)(ws + p.bt_hi);    // parameter branch: grad_T weights
  uint16_t* bt_lo = (uint16_t*)(ws + p.bt_lo);
  uint16_t* bx_hi = (uint16_t*)(ws + p.bx_hi);    // feature branch: grad_X weights
  uint16_t* bx_lo = (uint16_t*)(ws + p.bx_lo);
  uint32_t* gpk = (uint32_t*)(ws + p.gpk);
  // (the packed feature words the forward call left with the caller, se3conv_prepared, or this call's own)
  const bool have_featpk = prep && prep->feat_words && prep->feat_words_valid;
  uint32_t* featpk = prep && prep->feat_words ? prep->feat_words : (uint32_t*)(ws + p.featpk);
  uint32_t* bigw = (uint32_t*)big;
  uint32_t* u = (uint32_t*)(ws + p.u);
  const float inv_phi = inv_fin / kGeluOut;  // T and U hold kGeluOut * (the reference's values), see gelu_scaled
  pb.split(grad_out, gpk, rows_out * s->c_out);
  if (u_form) pb.weights(conv_weights, s->c_in, kb, s->c_out, 2, bx_hi, bx_lo, nullptr, 1.0f, false, p.fmt_u);
  if (want_params && !have_featpk) pb.split(feat, featpk, rows_in * s->c_in);
  if (p.grad_t)
    // alpha = nu/F_in is folded into these weights (one multiply per weight instead of one per grad_T element)
    pb.weights(conv_weights, s->c_in, kb, s->c_out, 1, bt_hi, bt_lo, nu, inv_fin, p.strip_t);
  if (int rc = pb.launch(stream)) return rc;
  // The sums that end the pass -- split-K partials of the grad_X GEMM, row-range partials of the weight-gradient GEMM,
  // per-workgroup partials of d[A; beta] -- write final outputs nobody in this call reads: one launch folds them all
  ReduceBatch final_sums;

  // One sequence of stages for every request, each behind its flag of the plan.  Writers first: the two kernels that write
  // a row-sized tensor (U, grad_T) go first, their readers after them.  Whatever runs right behind a ~1 GB writer is slowed
  // while the caches drain (a memory-bound reader by 15-30 %, whichever tensor it reads): in the order  U-writer, grad_X
  // GEMM, grad_T writer, parameter gradients  two readers sit in that position, here only one does (gemm_gradX 0.221 ->
  // 0.187 ms at the headline shape).
  if (u_form) {
    if (int rc = launch_edge_t_bf16("edge_t_transposed", gt, gpk, s->c_out, rows_out, axes_ext, rho, u, stream, p.fmt_u))
      return rc;
  }
  // The dense products.  On an under-filled level (BwdPlan::share_dense) those this call runs are the roles of ONE launch
  // right behind the U writer -- they read U, g, f and T and write grad_T, dX and the weight gradient's partials, nothing of
  // each other's -- and the launchers below only describe their product to `shared`; with one product left nothing is shared.
  DenseShare shared;
  ReduceBatch shared_sums;  // the partial sums of the shared roles: they join final_sums where those of separate launches do
  DenseShare* const share = p.share_dense && (int)p.grad_t + (int)u_form + (int)(grad_weights != nullptr) >= 2 ? &shared : nullptr;
  const uint32_t* t_rows = (const uint32_t*)t_save;  // the weight gradient's T, where it reads T
  auto recompute_t = [&]() -> int {
    if (!grad_weights || p.dw != WeightGrad::t_recomputed) return SE3_OK;
    uint32_t* tt = (uint32_t*)(ws + p.t);
    t_rows = tt;
    return launch_edge_t_bf16("edge_t_recompute", g, featpk, s->c_in, rows_in, axes_ext, rho, tt, stream, p.fmt_t);
  };
  auto grad_x = [&]() -> int {
    return launch_gemm_nn_bf16("gemm_gradX", u, bx_hi, bx_lo, grad_feat, false, rows_in, s->c_in, s->c_out * kb,
                               (float*)(ws + p.split_x), nu, inv_phi, stream, p.fmt_u, share ? &shared_sums : &final_sums, share);
  };
  auto grad_w = [&]() -> int {
    if (p.dw == WeightGrad::u)  // C'[(o,k), i] = sum_p U[p,(o,k)] f[p,i]; the batched reduction stores it as dW[i,k,o]
      return launch_gemm_tn_bf16("gemm_gradW", u, featpk, grad_weights, tn_partials, p.tn.splits, p.tn.m, p.tn.ka, p.tn.n, nu,
                                 inv_phi, stream, p.fmt_u, share ? &shared_sums : &final_sums, true, share);
    // dW[(i,k),o] = sum_m T[m,(i,k)] g[m,o]
    return launch_gemm_tn_bf16("gemm_gradW", t_rows, gpk, grad_weights, tn_partials, p.tn.splits, p.tn.m, p.tn.ka, p.tn.n, nu,
                               inv_phi, stream, p.fmt_t, share ? &shared_sums : &final_sums, false, share);
  };
  if (share) {  // (a recomputed T is an operand of the shared launch: written in front of it)
    if (int rc = recompute_t()) return rc;
    shared.next_order = 2;  // in the grid: the long k loops of grad_X first, the short strips of grad_T last
  }
  if (p.grad_t) {  // grad_T[m,(i,k)] = sum_o g[m,o] W'[i,k,o] into `big`
    if (int rc = p.strip_t ? launch_gemm_strip_bf16("gemm_gradT", gpk, bt_hi, bt_lo, bigw, rows_out, ck, s->c_out, stream, share)
                           : launch_gemm_nn_bf16("gemm_gradT", gpk, bt_hi, bt_lo, bigw, true, rows_out, ck, s->c_out,
                                                 (float*)(ws + p.split), nullptr, 1.0f, stream, 0, nullptr, share))
      return rc;
  }
  if (share) {
    shared.next_order = 0;
    if (u_form)
      if (int rc = grad_x()) return rc;
    shared.next_order = 1;
    if (grad_weights)
      if (int rc = grad_w()) return rc;
    if (int rc = shared.launch(stream)) return rc;
  }
  if (edge_major) {  // the feature gradient per frame-edge from grad_T, then its per-source sums
    float* d_rows = (float*)(ws + p.dx_rows);
    if (int rc = launch_edge_dx_bf16("edge_dx", g, axes_ext, rho, bigw, s->c_in, d_rows, stream)) return rc;
    if (int rc = launch_dx_gather_sum("dx_gather", d_rows, neighbors, ends, t_samples, t_ends, t_edge_ids, s->n_in, s->f_in * s->c_in,
                                      1.0f / kGeluOut, grad_feat, stream))
      return rc;
  }
  if (grad_axes || grad_biases) {
    // d[A; beta]: per-workgroup partial sums; their fixed-order reduction joins the batch (the bf16 kernels accumulate with
    // 2 GELU', gelu_scaled_grad: the 0.5 is applied there)
    int n_part = 0;
    if (int rc = launch_edge_param_grad_bf16("edge_param_grad", g, featpk, s->c_in, rows_in, axes_ext, rho, bigw, partials,
                                             p.n_param_partials, &n_part, stream))
      return rc;
    final_sums.params(partials, n_part, grad_axes, grad_biases, 0.5f);
  }
  for (int i = 0; i < shared_sums.jobs.count; ++i) final_sums.jobs.job[final_sums.jobs.count++] = shared_sums.jobs.job[i];
  if (!share) {
    if (u_form)
      if (int rc = grad_x()) return rc;
    if (int rc = recompute_t()) return rc;
    if (grad_weights)
      if (int rc = grad_w()) return rc;
  }
  return final_sums.launch(stream);
}

// Host only: the call itself with every launch replaced by its launcher's report (common.h: forms_only).  The pointers are
// one dummy address nobody dereferences; the workspace check is passed by claiming all of it.
extern "C" int se3conv_forms(const se3conv_shape* s, int pass, int want_feat, int want_params, int have_t, int cu_count, char* buf,
                             size_t len) {
  if (!shape_ok(s) || !buf || len == 0 || cu_count < 1 || (pass != SE3_PASS_FWD && pass != SE3_PASS_BWD)) return SE3_ERR_INVALID_ARGUMENT;
  alignas(256) static char dummy[256];
  float* const f = reinterpret_cast<float*>(dummy);
  int32_t* const i = reinterpret_cast<int32_t*>(dummy);
  FormSink sink;
  sink.n_cu = cu_count;
  t_forms = &sink;
  int rc;
  if (pass == SE3_PASS_FWD)
    rc = se3conv_fwd_prepared(f, f, f, f, i, i, f, f, f, f, f, f, s, f, have_t ? f : nullptr, dummy, SIZE_MAX, nullptr, nullptr);
  else
    rc = se3conv_bwd_prepared(f, f, f, f, i, i, i, i, i, f, f, f, f, f, f, have_t ? f : nullptr, f, s, want_feat ? f : nullptr,
                              want_params ? f : nullptr, want_params ? f : nullptr, want_params ? f : nullptr, dummy, SIZE_MAX,
                              nullptr, nullptr);
  t_forms = nullptr;
  if (rc != SE3_OK) return rc;
  if (sink.lines.size() + 1 > len) return SE3_ERR_WORKSPACE;
  std::memcpy(buf, sink.lines.c_str(), sink.lines.size() + 1);
  return SE3_OK;
}

// ---- optional per-kernel timing ------------------------------------------------------------------

namespace se3 {
namespace {
struct ProfRec { std::string tag; hipEvent_t start, stop; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::map<std::string, std::pair<double, int64_t>> g_prof_acc;
ProfRec* g_prof_open = nullptr;

void prof_drain_locked() {
  for (auto& r : g_prof_recs) {
    float ms = 0.f;
    if (hipEventSynchronize(r.stop) == hipSuccess && hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
      auto& a = g_prof_acc[r.tag];
      a.first += ms;
      a.second += 1;
    }
    (void)hipEventDestroy(r.start);
    (void)hipEventDestroy(r.stop);
  }
  g_prof_recs.clear();
}
}  // namespace

void prof_begin(const char* tag, hipStream_t stream) {
  if (!g_prof_on || forms_only()) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r;
  r.tag = tag;
  if (hipEventCreate(&r.start) != hipSuccess || hipEventCreate(&r.stop) != hipSuccess) return;
  (void)hipEventRecord(r.start, stream);
  g_prof_recs.push_back(r);
  g_prof_open = &g_prof_recs.back();
}

void prof_end(hipStream_t stream) {
  if (!g_prof_on || forms_only()) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_prof_open) (void)hipEventRecord(g_prof_open->stop, stream);
  g_prof_open = nullptr;
}
}  // namespace se3

extern "C" int se3_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(se3::g_prof_mu);
  if (!on) se3::prof_drain_locked();
  se3::g_prof_on = on != 0;
  return SE3_OK;
}

extern "C" int se3_profile_reset(void) {
  std::lock_guard<std::mutex> lk(se3::g_prof_mu);
  se3::prof_drain_locked();
  se3::g_prof_acc.clear();
  return SE3_OK;
}

extern "C" int se3_profile_read(const char* tag, double* total_ms, int64_t* launches) {
  if (!tag || !total_ms || !launches) return SE3_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(se3::g_prof_mu);
  se3::prof_drain_locked();
  auto it = se3::g_prof_acc.find(tag);
  *total_ms = it == se3::g_prof_acc.end() ? 0.0 : it->second.first;
  *launches = it == se3::g_prof_acc.end() ? 0 : it->second.second;
  return SE3_OK;
}

extern "C" int se3_profile_tags(char* buf, size_t len) {
  if (!buf || len == 0) return SE3_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(se3::g_prof_mu);
  se3::prof_drain_locked();
  std::string all;
  for (auto& kv : se3::g_prof_acc) all += (all.empty() ? "" : ",") + kv.first;
  if (all.size() + 1 > len) return SE3_ERR_WORKSPACE;
  std::memcpy(buf, all.c_str(), all.size() + 1);
  return SE3_OK;
}
