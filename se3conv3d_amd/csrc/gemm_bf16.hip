// Split-bf16 GEMMs (v_mfma_f32_32x32x16_bf16, 3 products per multiply, fp32 accumulate).
//
//   gemm_nn_bf16 : C[M,N]  = alpha * A[M,K] @ B[K,N]     A = packed words (hi<<16|lo), row-major;
//                  B = the layer's weights, pre-split by prep_weights_kernel into two bf16 planes
//                  stored transposed, Bt[N][Kp] (Kp = K rounded up to 32, zero padded), so that an
//                  MFMA B fragment (8 consecutive k of one column) is one 16-byte LDS read.
//   gemm_tn_bf16 : C[Ka,N] = alpha * A[M,Ka]^T @ B[M,N]  both packed words; reduction over the rows
//                  (weight gradient).  The k-strided operands go through LDS and are read by column.
//
// These are streaming kernels: A (1 GB at the headline shape) is read once, so they are HBM-bound
// as long as the MFMA side reaches ~1/3 of its peak.
//
// The three NN kernels (gemm_nn_bf16 over packed words, gemm_nn_t24 over 3-byte rows, gemm_nn_t16 over 2.25-byte block rows)
// are one skeleton; what they share is written once (profiles/gemm_nn_pieces.txt has the device code it was checked against):
//   piece                                   gemm_nn_bf16          gemm_nn_t24        gemm_nn_t16
//   weight_plane_rsrc                       yes                   yes                yes
//   weight passes: the loads                own (32-k tiles,      own text           own text    (every shared shape moved
//                                           other thread map)                                    the waits of a k loop)
//   nn_store_weights_half                   own store_tile        yes                yes
//   A fragments out of LDS                  pair_hi / pair_lo     t24_lo_word        straight reads
//   nn_mfma_tiles                           yes                   yes                yes
//   nn_store_acc                            yes                   yes                yes
// gemm_tn_bf16: the row-plane forms (AFMT 1, 2) share store_b_planes; their B loads are written in both branches, in front of
// the A loads (behind them the address selects compile differently and the stage loop's waits move).  gemm_a_row_bytes is
// the size of an A row for the kernels and the host.
#include <atomic>

#include "common.h"

#define SE3_GRID_BLOCK blockIdx  // the stand-alone kernels: see gemm_nn_bf16_body.h

namespace se3 {

namespace {

constexpr int kGemmDepth = 4;  // k-tiles of A in flight in gemm_nn_bf16_kernel (3, 4, 6 and 8 measured the same, see there)
constexpr int BM = 128, BN = 64, BK = 32;
constexpr int A_LD = BK + 4;   // words; 144-byte pitch keeps 16-byte alignment and spreads ds_read_b128 over all banks
constexpr int B_LD = BK + 8;   // bf16;  80-byte pitch, same properties

// bytes of one A row of k values by its format: 0 packed words, 1 the 3-byte rows (T24: k * 3 = t24_row_bytes(k / kBasis)
// for the k the format exists for, and exact for any other k a caller asks about before its form is checked), 2 the
// 2.25-byte block rows (T16, whole blocks of 32: the forms reject other k)
__host__ __device__ inline int64_t gemm_a_row_bytes(int afmt, int k) {
  return afmt == 2 ? t16_row_bytes(k / kBasis) : (int64_t)k * (afmt == 1 ? 3 : 4);
}

// up to 4 consecutive words starting at p, `avail` of them readable (<= 0: none).  Native vector
// type on purpose: HIP's uint4 struct made the register tiles of the pipeline land in scratch.
__device__ __forceinline__ u32x4 ld4_words(const uint32_t* p, int64_t avail, bool vec) {
  if (avail >= 4 && vec) return *reinterpret_cast<const u32x4*>(p);
  const uint32_t x = avail > 0 ? p[0] : 0u, y = avail > 1 ? p[1] : 0u, z = avail > 2 ? p[2] : 0u,
                 w = avail > 3 ? p[3] : 0u;
  return u32x4{x, y, z, w};
}

// Where a workgroup stands in its grid: HwGrid is the launch's own grid (a stand-alone kernel), VirtGrid a role's virtual
// grid inside the shared launch of backward's dense products (bwd_dense_shared_kernel).  The strip GEMM's body is a function
// over one of these (it compiles to the same device code as the kernel it was); the bodies with LDS tiles are included
// texts (gemm_nn_bf16_body.h) that read SE3_GRID_BLOCK.
struct HwGrid {
  __device__ __forceinline__ unsigned bx() const { return blockIdx.x; }
  __device__ __forceinline__ unsigned by() const { return blockIdx.y; }
  __device__ __forceinline__ unsigned bz() const { return blockIdx.z; }
  __device__ __forceinline__ unsigned gdy() const { return gridDim.y; }
};
struct VirtGrid {
  unsigned x, y, z, ny;
  __device__ __forceinline__ unsigned bx() const { return x; }
  __device__ __forceinline__ unsigned by() const { return y; }
  __device__ __forceinline__ unsigned bz() const { return z; }
  __device__ __forceinline__ unsigned gdy() const { return ny; }
};

// ---- Pieces the NN kernels share (who takes which: the table in the header comment) -------------------------------------

// one plane of the prepared weights, Bt[n][kp] bf16, as a buffer resource; !bounded: the guarded-load form, which takes no buffer load
__device__ __forceinline__ __amdgpu_buffer_rsrc_t weight_plane_rsrc(const uint16_t* bt, int n, int kp, bool bounded = true) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(bt), (short)0,
                                           bounded ? (int)(uint32_t)((int64_t)n * kp * 2) : 0, 0x00020000);
}

// The weights of a 64-k super tile (the kernels over row planes) are loaded in 2 * NB passes of kWeightPassCols columns per
// plane, into bh[] / bl[]; passes alternate which 32-k half a thread holds (each kernel's load_super).  This writes one
// half to LDS buffer `buf`.  The passes come in pairs (2 g, 2 g + 1): the even pass holds this thread's piece of the half
// iff !q (q = half ^ bit 2 of tid); row r8 = tid >> 3 of the pass, column c4 = (tid & 3) * 8.  LDS: the kernel's tile
// image as it declares it, [2][64 NB][B_LD] (an array or a pointer to its first buffer: no decay, the addressing stays the
// kernel's own).
constexpr int kWeightPassCols = 32;
template <int NB, class LDS>
__device__ __forceinline__ void nn_store_weights_half(const u32x4 (&bh)[2 * NB], const u32x4 (&bl)[2 * NB], LDS& bsh, LDS& bsl,
                                                      int buf, bool q, int r8, int c4) {
  constexpr int CP = kWeightPassCols;
#pragma unroll
  for (int g = 0; g < NB; ++g) {
    *reinterpret_cast<u32x4*>(&bsh[buf][CP * (2 * g) + (q ? CP : 0) + r8][c4]) = q ? bh[2 * g + 1] : bh[2 * g];
    *reinterpret_cast<u32x4*>(&bsl[buf][CP * (2 * g) + (q ? CP : 0) + r8][c4]) = q ? bl[2 * g + 1] : bl[2 * g];
  }
}

// The A fragments of k-step kk against the wavefront's 2 * NB column tiles of LDS buffer `buf`.
template <int NB, class LDS>
__device__ __forceinline__ void nn_mfma_tiles(u32x4 a_hi, u32x4 a_lo, const LDS& bsh, const LDS& bsl, int buf, int kk, int rl,
                                              f32x16 (&acc)[2 * NB]) {
#pragma unroll
  for (int ct = 0; ct < 2 * NB; ++ct) {
    const u32x4 bh = *reinterpret_cast<const u32x4*>(&bsh[buf][32 * ct + rl][kk]);
    const u32x4 bl = *reinterpret_cast<const u32x4*>(&bsl[buf][32 * ct + rl][kk]);
    acc[ct] = mfma_bf16x3(a_hi, a_lo, bh, bl, acc[ct]);
  }
}

// The accumulators of a wavefront (rows m0 + 32 wave .., columns n0 ..) -> C.
// OUT_MODE 0: fp32 C * alpha, 1: packed words of C * alpha, 2: raw fp32 partial of split bz (the workgroup's z index; no alpha).
template <int OUT_MODE, int NB>
__device__ __forceinline__ void nn_store_acc(const f32x16 (&acc)[2 * NB], void* c, int64_t m, int n, int64_t m0, int n0,
                                             int wave, int rl, int h, const float* alpha_num, float alpha_scale, unsigned bz) {
  const float alpha = OUT_MODE == 2 ? 1.0f : (alpha_num ? *alpha_num : 1.0f) * alpha_scale;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t gr = m0 + wave * 32 + acc_row(r, h);
    if (gr < m) {
#pragma unroll
      for (int ct = 0; ct < 2 * NB; ++ct) {
        const int gc = n0 + 32 * ct + rl;
        if (gc >= n) continue;
        if constexpr (OUT_MODE == 1) {
          static_cast<uint32_t*>(c)[gr * n + gc] = split_pack(alpha * acc[ct][r]);
        } else {
          float* out = static_cast<float*>(c) + (OUT_MODE == 2 ? (int64_t)bz * m * n : 0);
          out[gr * n + gc] = alpha * acc[ct][r];
        }
      }
    }
  }
}

// OUT_MODE: see nn_store_acc.
// The A stream is prefetched DEPTH k-tiles ahead in registers: one k-tile of compute (~400 cycles) is
// far shorter than an HBM round trip, so a single tile in flight leaves the kernel latency-bound.
// FAST (k % 32 == 0, operands < 4 GB): every load is an unconditional raw buffer load whose out-of-range
// lanes return 0 -- no branches around the loads, so the compiler keeps all three tiles in flight (with
// guarded loads it drained vmcnt(0) after every tile and the kernel ran at half the HBM rate).
// NB = 64-column blocks per workgroup: 1 for N <= 64; 2 (128 columns, 4 column tiles per wavefront) for wider
// outputs, where the products turn MFMA-bound (24 instead of 12 MFMAs per A fragment set and k-tile).
template <int OUT_MODE, bool FAST, int NB>
__global__ __launch_bounds__(256) void gemm_nn_bf16_kernel(const uint32_t* __restrict__ a,
                                                           const uint16_t* __restrict__ bt_hi,
                                                           const uint16_t* __restrict__ bt_lo, void* __restrict__ c,
                                                           int64_t m, int n, int k, int kp, int kt_per_split,
                                                           const float* __restrict__ alpha_num, float alpha_scale) {
  __shared__ __attribute__((aligned(16))) uint32_t as[2][BM][A_LD];
  constexpr int BNW = BN * NB;  // columns per workgroup
  __shared__ __attribute__((aligned(16))) uint16_t bsh[2][BNW][B_LD];
  __shared__ __attribute__((aligned(16))) uint16_t bsl[2][BNW][B_LD];
#include "gemm_nn_bf16_body.h"
}

// NN GEMM over A rows in the 3-byte format (common.h, T24; k a multiple of 64).  What bounds the A stream of these
// products is the number of 64-byte requests, not the bytes (tools/probes/tile_read3.hip: 6144-byte rows read 64 + 32
// bytes at a time take as long as 8192-byte rows read 128 bytes at a time), so the loads work on "super tiles" of 64
// k: 128 B of hi and 64 B of lo per row and instruction.  LDS and the MFMA stage keep the 32-k tiles of the kernel
// above: the two halves of a super tile are the two LDS buffers.  Lane l of load p reads 16-byte column
// (l & 7) ^ (4 * (p & 1)), so every thread holds as many pieces of either half and the stores stay full-width.
// (Measured and not kept: row blocks last-written first -- no difference; the row stream loaded non-temporally -- slower.)
// (256-row workgroups -- 8 wavefronts, the weight planes fetched from L2 half as often -- were measured in round 3:
// nothing at the headline shape, 15 % slower on a 150 k-row scene whose 586 workgroups no longer divide into full rounds:
// profiles/r03_gemm_256row_ab.txt.)
// (Two k groups per workgroup -- eight wavefronts, each group walking half of the super tiles, the partial tiles added
// through LDS -- were measured in round 5 against the split over grid.z: no faster, profiles/r05_nn_kgroups_ab.txt.)
template <int OUT_MODE, int NB>
__global__ __launch_bounds__(256) void gemm_nn_t24_kernel(const uint8_t* __restrict__ a,
                                                          const uint16_t* __restrict__ bt_hi,
                                                          const uint16_t* __restrict__ bt_lo, void* __restrict__ c,
                                                          int64_t m, int n, int k, int st_per_split,
                                                          const float* __restrict__ alpha_num, float alpha_scale) {
#include "gemm_nn_t24_body.h"
}

// LDS of gemm_nn_bf16_kernel: the A image, then the two weight images of nb 64-column blocks (nb = 0: the A image alone)
constexpr int gemm_nn_bf16_lds_bytes(int nb) { return 2 * BM * A_LD * 4 + 2 * (2 * BN * nb * B_LD * 2); }
constexpr int gemm_nn_t24_lds_bytes(int nb) {
  return 2 * BM * (BK + 8) * 2 + 2 * BM * (BK + 16) + 2 * (2 * BN * nb * B_LD * 2);
}

// NN GEMM over A rows in the 2.25-byte block format (common.h, T16; k a multiple of 256 = one mega tile of the exponent
// plane).  Same skeleton as the 3-byte kernel above -- super tiles of 64 k, the two 32-k halves of a super tile are the
// two LDS buffers -- with these differences: the row stream is the mantissa plane (128 B per row and super tile, as the
// 3-byte format's hi plane) plus ONE 8-byte exponent load per thread and mega tile (4 super tiles; the 8 threads of a
// row read one 64-byte line); a piece (8 mantissas = 2 blocks) is decoded to its hi / lo bf16 planes on the way into
// LDS (t16_unpack2: 5.5 VALU per element, once per element of A -- the MFMA stage then reads both fragments as they
// lie, no rebuild); no per-block phase stagger (4608-byte rows do not alias onto a few channels as 8192-byte rows do).
template <int OUT_MODE, int NB>
__global__ __launch_bounds__(256) void gemm_nn_t16_kernel(const uint8_t* __restrict__ a,
                                                          const uint16_t* __restrict__ bt_hi,
                                                          const uint16_t* __restrict__ bt_lo, void* __restrict__ c,
                                                          int64_t m, int n, int k, int st_per_split,
                                                          const float* __restrict__ alpha_num, float alpha_scale) {
  constexpr int BNW = BN * NB;
  constexpr int RB = BM;           // rows per workgroup
  constexpr int RP = 32;           // rows one load pass covers (8 threads per row): 4 passes = RB rows
  constexpr int CP = kWeightPassCols, NBP = 2 * NB;
  __shared__ __attribute__((aligned(16))) uint16_t ash[2][RB][BK + 8];   // 80-byte pitch
  __shared__ __attribute__((aligned(16))) uint16_t asl[2][RB][BK + 8];
  __shared__ __attribute__((aligned(16))) uint16_t bsh[2][BNW][B_LD];
  __shared__ __attribute__((aligned(16))) uint16_t bsl[2][BNW][B_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * RB;
  const int n0 = blockIdx.y * BNW;
  const int st_begin = blockIdx.z * st_per_split;          // a multiple of 4 (host)
  const int ns = min(k / 64 - st_begin, st_per_split);     // super tiles of this block (> 0, a multiple of 4)

  struct Super { u32x4 am[4], bh[NBP], bl[NBP]; };
  const uint32_t rb = (uint32_t)k / 32u * 72u;             // row bytes: 2 k of mantissas + k / 4 exponent bytes
  const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a), (short)0, (int)(uint32_t)(m * rb), 0x00020000);
  const __amdgpu_buffer_rsrc_t bh_rs = weight_plane_rsrc(bt_hi, n, k), bl_rs = weight_plane_rsrc(bt_lo, n, k);
  const int hsel = (tid >> 2) & 1;
  // lane l of load pass p reads 16-byte column (l & 7) ^ (4 * (p & 1)) of its row (see gemm_nn_t24_kernel)
  auto load_super = [&](Super& t, int st) {
    const uint32_t k0 = (uint32_t)(st_begin + st) * 64u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t off = (uint32_t)(m0 + p * RP + (tid >> 3)) * rb + k0 * 2u + (uint32_t)((tid & 7) ^ ((p & 1) << 2)) * 16u;
      t.am[p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, off, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < NBP; ++j) {  // pass j: columns CP * j + (tid >> 3); passes alternate which 32-k half a thread holds
      const uint32_t off = ((uint32_t)(n0 + CP * j + (tid >> 3)) * (uint32_t)k + k0 + (uint32_t)((tid & 7) ^ ((j & 1) << 2)) * 8u) * 2u;
      t.bh[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(bh_rs, off, 0, 0));
      t.bl[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(bl_rs, off, 0, 0));
    }
  };
  // exponents of this thread's pieces for the 4 super tiles of mega tile `mg` (relative to st_begin): pass p, piece
  // (tid & 7) ^ (4 (p & 1)) -> 8 bytes = [super tile s][block of the piece]
  auto load_exps = [&](u32x2 (&e)[4], int mg) {
    const uint32_t e0 = (uint32_t)k * 2u + (uint32_t)(st_begin / 4 + mg) * 64u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t off = (uint32_t)(m0 + p * RP + (tid >> 3)) * rb + e0 + (uint32_t)((tid & 7) ^ ((p & 1) << 2)) * 8u;
      e[p] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(a_rs, off, 0, 0));
    }
  };
  // the 32-k half `hf` of super tile number s (0..3) of its mega tile -> LDS buffer `buf`
  auto store_half = [&](const Super& t, const u32x2 (&e)[4], int s, int hf, int buf) {
    const bool q = (hf ^ hsel) != 0;
    const int r8 = tid >> 3, c4 = (tid & 3) * 8;
#pragma unroll
    for (int g = 0; g < 2; ++g) {  // the two passes whose piece lies in this half: p = 2 g + q
      const u32x4 mw = q ? t.am[2 * g + 1] : t.am[2 * g];
      const u32x2 ev = q ? e[2 * g + 1] : e[2 * g];
      const uint32_t e2 = (s < 2 ? ev[0] : ev[1]) >> (16 * (s & 1));  // bytes 2 s, 2 s + 1 of the 8
      u32x4 vh, vl;
      t16_unpack8(mw, e2, vh, vl);
      const int row = (2 * g + (q ? 1 : 0)) * RP + r8;
      *reinterpret_cast<u32x4*>(&ash[buf][row][c4]) = vh;
      *reinterpret_cast<u32x4*>(&asl[buf][row][c4]) = vl;
    }
    nn_store_weights_half<NB>(t.bh, t.bl, bsh, bsl, buf, q, r8, c4);
  };
  f32x16 acc[2 * NB];
#pragma unroll
  for (int ct = 0; ct < 2 * NB; ++ct) acc[ct] = zero16();
  auto compute = [&](int buf) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kk = 16 * s + 8 * h;
      const u32x4 a_hi = *reinterpret_cast<const u32x4*>(&ash[buf][wave * 32 + rl][kk]);
      const u32x4 a_lo = *reinterpret_cast<const u32x4*>(&asl[buf][wave * 32 + rl][kk]);
      nn_mfma_tiles<NB>(a_hi, a_lo, bsh, bsl, buf, kk, rl, acc);
    }
  };
  // Mega tile = 4 super tiles, fully unrolled (the exponent bytes of super tile s sit at a compile-time position of the
  // thread's 8).  Two super tiles in registers; the next mega tile's exponents are requested during super tile 1 and are
  // first needed when super tile 3 hands over to the next mega tile's super tile 0.
  Super t0, t1;
  u32x2 ex[4], ex_next[4];
  load_exps(ex, 0);
  load_super(t0, 0);
  load_super(t1, 1);
  store_half(t0, ex, 0, 0, 0);
  __syncthreads();
  const int n_mega = ns / 4;
  for (int mg = 0; mg < n_mega; ++mg) {
    const int st = 4 * mg;
    const bool more = mg + 1 < n_mega;
    // super tile 0 (in t0)
    compute(0);
    store_half(t0, ex, 0, 1, 1);
    __syncthreads();
    load_super(t0, st + 2);
    compute(1);
    store_half(t1, ex, 1, 0, 0);
    __syncthreads();
    // super tile 1 (in t1)
    compute(0);
    store_half(t1, ex, 1, 1, 1);
    __syncthreads();
    load_super(t1, st + 3);
    if (more) load_exps(ex_next, mg + 1);
    compute(1);
    store_half(t0, ex, 2, 0, 0);
    __syncthreads();
    // super tile 2 (in t0)
    compute(0);
    store_half(t0, ex, 2, 1, 1);
    __syncthreads();
    if (more) load_super(t0, st + 4);
    compute(1);
    store_half(t1, ex, 3, 0, 0);
    __syncthreads();
    // super tile 3 (in t1)
    compute(0);
    store_half(t1, ex, 3, 1, 1);
    __syncthreads();
    if (more) load_super(t1, st + 5);
    compute(1);
    if (more) {
#pragma unroll
      for (int p = 0; p < 4; ++p) ex[p] = ex_next[p];
      store_half(t0, ex, 0, 0, 0);
    }
    __syncthreads();
  }

  nn_store_acc<OUT_MODE, NB>(acc, c, m, n, m0, n0, wave, rl, h, alpha_num, alpha_scale, blockIdx.z);
}

// Row-strip GEMM for the wide, write-dominated products with a short k (grad_T = g W^T, H = f W''):
//   C[m, n] (packed words) = A[m, k] (packed words) * Bt[n, k]^T,   k <= 64, n large (C_in*K or C_out*K = 2048)
// A wavefront keeps its 32 rows of A as MFMA fragments for the whole kernel and walks the n range 32 columns
// at a time: 3*KS MFMAs, then 16 results per lane are split to hi/lo and stored (128 contiguous bytes per
// row and half-wave).  The next tile's weight fragments (L1/L2-resident, 0.5 MB in all) are requested as soon
// as the MFMAs have issued and land during the epilogue.  Everything fits 128 VGPRs, so 4 wavefronts share a
// SIMD and the 4096 strips of the headline shape are resident at once (the previous 64-column version needed
// ~150 VGPRs: 3 per SIMD, i.e. a second, mostly empty round).  alpha is folded into the prepared weights.
constexpr int kStripRot = 17;  // column tiles a strip's walk starts further on than its predecessor's ("Column order rotated" below)
// (body and stand-alone kernel: see HwGrid)
template <int KS, class G>  // kp / 16: 2, 4 (k <= 64, 120 VGPRs) or 8 (k <= 128: twice the fragments, 3 waves per SIMD)
__device__ __forceinline__ void gemm_strip_bf16_body(const G g, const uint32_t* a,
                                                     const uint16_t* bt_hi, const uint16_t* bt_lo,
                                                     uint32_t* c, int64_t m, int n, int k) {
  constexpr int KP = KS * 16;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform: feeds a buffer descriptor
  const int rl = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)g.bx() * 128 + wave * 32;
  if (row0 >= m) return;
  const __amdgpu_buffer_rsrc_t a_rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a), (short)0, (int)(uint32_t)(m * k * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t bh_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(bt_hi), (short)0, (int)(uint32_t)((int64_t)n * KP * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t bl_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(bt_lo), (short)0, (int)(uint32_t)((int64_t)n * KP * 2), 0x00020000);

  u32x4 a_hi[KS], a_lo[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int kk = 16 * ks + 8 * h;
    uint32_t w[8];
    if (k % 8 == 0) {  // block-uniform: whole 8-word groups are inside or outside the row
      const uint32_t off = kk < k ? (uint32_t)(((row0 + rl) * k + kk) * 4) : 0xfffffff0u;
      const auto v0 = __builtin_amdgcn_raw_buffer_load_b128(a_rs, off, 0, 0);
      const auto v1 = __builtin_amdgcn_raw_buffer_load_b128(a_rs, kk < k ? off + 16 : 0xfffffff0u, 0, 0);
      w[0] = v0[0], w[1] = v0[1], w[2] = v0[2], w[3] = v0[3], w[4] = v1[0], w[5] = v1[1], w[6] = v1[2], w[7] = v1[3];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        w[j] = __builtin_amdgcn_raw_buffer_load_b32(
            a_rs, kk + j < k ? (uint32_t)(((row0 + rl) * k + kk + j) * 4) : 0xfffffff0u, 0, 0);
    }
    frags_from_words(w, a_hi[ks], a_lo[ks]);
  }

  // Weight fragments of the next 32 columns.  The loads are issued through inline asm and waited for with an
  // explicit counted s_waitcnt: vmcnt retires loads and stores in order on this chip, so "at most 16 outstanding"
  // after the 16 stores of a tile means the 2*KS older loads have landed while the stores are still in flight.
  // (The compiler's own wait insertion treats mixed loads/stores as unordered and emits vmcnt(0): every tile
  // then waits for its stores to retire, which is what bounded the first version of this kernel.)
  u32x4 bh[KS], bl[KS];
  auto load_b = [&](int n0) {
    const uint32_t off = (uint32_t)(((n0 / 32) * KS * 64 + lane) * 16);  // fragment-ordered planes, 1 KB per k-step
    const uint32_t off4 = off + 4096u;  // the instruction's immediate offset has 12 bits: k-steps 4.. go through here
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3"
                   : "+v"(bh[ks])
                   : "v"(ks < 4 ? off : off4), "s"(bh_rs), "n"(1024 * (ks & 3))
                   : "memory");
      asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3"
                   : "+v"(bl[ks])
                   : "v"(ks < 4 ? off : off4), "s"(bl_rs), "n"(1024 * (ks & 3))
                   : "memory");
    }
  };
  static_assert(KS == 2 || KS == 4 || KS == 8, "operand lists of SE3_WAIT_B");
#define SE3_WAIT_B(CNT)                                                                                           \
  do {                                                                                                            \
    if constexpr (KS == 2)                                                                                        \
      asm volatile("s_waitcnt vmcnt(" #CNT ")" : "+v"(bh[0]), "+v"(bh[1]), "+v"(bl[0]), "+v"(bl[1])::"memory");   \
    else if constexpr (KS == 4)                                                                                   \
      asm volatile("s_waitcnt vmcnt(" #CNT ")"                                                                    \
                   : "+v"(bh[0]), "+v"(bh[1]), "+v"(bh[KS - 2]), "+v"(bh[KS - 1]), "+v"(bl[0]), "+v"(bl[1]),      \
                     "+v"(bl[KS - 2]), "+v"(bl[KS - 1])::"memory");                                               \
    else                                                                                                          \
      asm volatile("s_waitcnt vmcnt(" #CNT ")"                                                                    \
                   : "+v"(bh[0]), "+v"(bh[1]), "+v"(bh[2]), "+v"(bh[3]), "+v"(bh[KS - 4]), "+v"(bh[KS - 3]),      \
                     "+v"(bh[KS - 2]), "+v"(bh[KS - 1]), "+v"(bl[0]), "+v"(bl[1]), "+v"(bl[2]), "+v"(bl[3]),      \
                     "+v"(bl[KS - 4]), "+v"(bl[KS - 3]), "+v"(bl[KS - 2]), "+v"(bl[KS - 1])::"memory");           \
  } while (0)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) bh[ks] = bl[ks] = u32x4{0u, 0u, 0u, 0u};
  // Output through a buffer descriptor based at the strip: rows >= m fall outside num_records and are dropped by
  // the hardware, the uniform part of every address ((row-of-register * n + n0) * 4) rides in the scalar offset, so
  // a store costs no VALU.  Straight-line loop body: the wait in front of the MFMAs must cover only the weight
  // loads, not the 16 younger stores (vmcnt counts both, in order) -- with per-store branches the compiler fell
  // back to vmcnt(0) and every tile waited for its stores to retire.
  const int64_t c_bytes = (m - row0) * (int64_t)n * 4;
  const __amdgpu_buffer_rsrc_t c_rs = __builtin_amdgcn_make_buffer_rsrc(
      c + row0 * n, (short)0, (int)(uint32_t)(c_bytes > 0xffffffffll ? 0xffffffffll : c_bytes), 0x00020000);
  const int voff = (4 * h * n + rl) * 4;
  const bool cols_full = n % 32 == 0;  // uniform
  // Column order rotated per strip: with a power-of-two row pitch (n * 4 = 8 KB) every wavefront of the chip would
  // otherwise write the same 128-byte column window of its rows at the same time, i.e. all traffic of a moment
  // lands on a handful of L2 / HBM channels.
  // the block's y index selects a contiguous range of column tiles (small M: the row strips alone cannot fill the chip)
  const int n_tiles_all = (n + 31) / 32;
  const int per = (n_tiles_all + (int)g.gdy() - 1) / (int)g.gdy();
  const int tile_lo = (int)g.by() * per;
  const int n_tiles = min(per, n_tiles_all - tile_lo);
  if (n_tiles <= 0) return;
  const int n_lo = tile_lo * 32, n_hi = min(n, (tile_lo + n_tiles) * 32);
  int n0 = n_lo + (int)(((g.bx() * 4 + wave) * (unsigned)kStripRot) % (unsigned)n_tiles) * 32;
  load_b(n0);
  SE3_WAIT_B(0);
  // (rotating wave priority, common.h rotate_priority, was measured here too -- every strip is resident for the whole
  // launch -- and loses 2 %: the kernel is bound by its stores, not by issue slots; profiles/r06_rotate_priority_ab.txt)
  for (int it = 0; it < n_tiles; ++it) {
    f32x16 acc = zero16();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = mfma_bf16x3(a_hi[ks], a_lo[ks], bh[ks], bl[ks], acc);
    const int n_next = n0 + 32 < n_hi ? n0 + 32 : n_lo;
    load_b(n_next);  // in flight during the epilogue below (after the last tile: one unused fetch)
    const int lane_off = (cols_full || n0 + rl < n) ? voff : (int)0x7fffff00;  // columns >= n: dropped
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      uint32_t w0, w1;
      split_pack2(acc[r], acc[r + 1], w0, w1);
      __builtin_amdgcn_raw_buffer_store_b32(w0, c_rs, lane_off, (acc_row(r, 0) * n + n0) * 4, 0);
      __builtin_amdgcn_raw_buffer_store_b32(w1, c_rs, lane_off, (acc_row(r + 1, 0) * n + n0) * 4, 0);
    }
    SE3_WAIT_B(16);  // the loads are older than the 16 stores
    n0 = n_next;
  }
#undef SE3_WAIT_B
}

template <int KS>
__global__ __launch_bounds__(256, KS <= 4 ? 4 : 2) void gemm_strip_bf16_kernel(const uint32_t* __restrict__ a,
                                                                 const uint16_t* __restrict__ bt_hi,
                                                                 const uint16_t* __restrict__ bt_lo,
                                                                 uint32_t* __restrict__ c, int64_t m, int n, int k) {
  gemm_strip_bf16_body<KS>(HwGrid{}, a, bt_hi, bt_lo, c, m, n, k);
}

// out = alpha * sum_z partials[z]  (fp32 or packed words)
template <bool OUT_PACKED>
__global__ void reduce_splits_kernel(const float* __restrict__ partials, void* __restrict__ out, int64_t count,
                                     int splits, const float* __restrict__ alpha_num, float alpha_scale) {
  const float alpha = (alpha_num ? *alpha_num : 1.0f) * alpha_scale;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
#pragma unroll 8
    for (int z = 0; z < splits; ++z) s += partials[(int64_t)z * count + i];
    if constexpr (OUT_PACKED) static_cast<uint32_t*>(out)[i] = split_pack(alpha * s);
    else static_cast<float*>(out)[i] = alpha * s;
  }
}

// One block: 128 (ka) x 64 (n) outputs over rows [split*chunk, (split+1)*chunk) in stages of 32 rows.
// FAST (n % 4 == 0, operands < 4 GB): unconditional raw buffer loads bounded at the split's last row (rows
// past it and columns past ka / n read as 0), stages prefetched 3 deep in registers like gemm_nn.
// AFMT 1: A rows in the 3-byte format (common.h, T24; ka a multiple of 64); the partial rows are written at t24_k_of().
// AFMT 2: A rows in the 2.25-byte block format (T16; ka a multiple of 128): a stage reads 256 B of mantissas per row
// and the two exponent bytes of every thread's piece, decodes to the same hi / lo 16-bit images (the lo plane is then
// the bf16 lo operand itself: no rebuild in the MFMA stage); partial rows at t16_k_of().
// The six LDS images of gemm_tn_bf16_kernel<., AFMT> as one buffer (the shared launch carves them from its dynamic LDS)
template <int AFMT>
struct TnLds {
  static constexpr int kARows = AFMT != 0 ? 1 : BK, kPRows = AFMT != 0 ? BK : 1, kAPitch = 128 + 32, kBPitch = BN + 32;
  static constexpr int o_ath = 2 * kARows * 128 * 4, o_atl = o_ath + 2 * kPRows * kAPitch * 2, o_bt = o_atl + 2 * kPRows * kAPitch * 2,
                       o_bth = o_bt + 2 * kARows * BN * 4, o_btl = o_bth + 2 * kPRows * kBPitch * 2, bytes = o_btl + 2 * kPRows * kBPitch * 2;
};
template <bool FAST, int AFMT>
__global__ __launch_bounds__(256) void gemm_tn_bf16_kernel(const uint32_t* __restrict__ a,
                                                           const uint32_t* __restrict__ b,
                                                           float* __restrict__ partials, int64_t m, int ka, int n,
                                                           int64_t chunk) {
  constexpr bool A16 = AFMT == 2;
  constexpr bool A24 = AFMT != 0;  // "the A operand comes as two 16-bit planes": everything below that is not format-specific
  static_assert(!A24 || FAST, "the 3-byte / T16 A formats are only read through buffer loads");
  // A24: hi / lo planes of A (lo bytes widened to 16 bits) and of B as 16-bit images whose rows are the K index of
  // the MFMAs; the fragments come out of ds_read_b64_tr_b16 (common.h) ready-made: 12 LDS reads and no v_perm per
  // k-step where gathering them with scalar reads took 32 reads + 24 v_perm.  Row pitches of 16 (mod 64) dwords
  // keep the 4-row blocks of a half-wavefront on distinct banks.
  constexpr int APITCH = 128 + 32, BPITCH = BN + 32;  // 320- and 192-byte rows
  __shared__ __attribute__((aligned(16))) uint32_t at[2][A24 ? 1 : BK][128];
  __shared__ __attribute__((aligned(16))) uint16_t ath[2][A24 ? BK : 1][APITCH];
  __shared__ __attribute__((aligned(16))) uint16_t atl[2][A24 ? BK : 1][APITCH];
  __shared__ __attribute__((aligned(16))) uint32_t bt[2][A24 ? 1 : BK][BN];
  __shared__ __attribute__((aligned(16))) uint16_t bth[2][A24 ? BK : 1][BPITCH];
  __shared__ __attribute__((aligned(16))) uint16_t btl[2][A24 ? BK : 1][BPITCH];
#include "gemm_tn_bf16_body.h"
}

// Bt[nn][kk] (two bf16 planes, pitch kp) from the layer weights W[C_in, K, C_out]:
//   mode 0 (out = T W)      : nn = o,          kk = i*K + k     value W[i,k,o]
//   mode 1 (gT = g W^T)     : nn = i*K + k,    kk = o           value W[i,k,o]
//   mode 2 (dX = U W')      : nn = i,          kk = o*K + k     value W[i,k,o]
//   mode 3 (H = f W'')      : nn = o*K + k,    kk = i           value W[i,k,o]
__global__ void prep_weights_kernel(const float* __restrict__ w, int c_in, int kb, int c_out, int mode, int n, int k,
                                    int kp, uint16_t* __restrict__ bt_hi, uint16_t* __restrict__ bt_lo,
                                    const float* __restrict__ scale_num, float scale, int frag) {
  const int64_t total = (int64_t)n * kp;
  const float sc = (scale_num ? *scale_num : 1.0f) * scale;  // the GEMM's alpha, applied to the weights once
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int nn = (int)(idx / kp), kk = (int)(idx % kp);
    float v = 0.f;
    if (kk < k) {
      if (mode == 0) v = w[(int64_t)kk * c_out + nn];
      else if (mode == 1) v = w[(int64_t)nn * c_out + kk];
      else if (mode == 2) v = w[((int64_t)nn * kb + (kk % kb)) * c_out + kk / kb];
      else v = w[((int64_t)kk * kb + (nn % kb)) * c_out + nn / kb];
    }
    const uint32_t pk = split_pack(v * sc);
    // frag layout (gemm_strip_bf16_kernel): the 16 bytes lane (nn % 32, (kk % 16) / 8) needs for k-step kk / 16 of
    // column tile nn / 32 sit at [tile][k-step][lane][8], so one load instruction reads 1 KB of consecutive bytes
    // (row-major planes make it touch 32 cache lines for the same 1 KB)
    const int64_t o = frag ? ((((int64_t)(nn / 32) * (kp / 16) + kk / 16) * 64 + ((kk % 16) / 8) * 32 + nn % 32) * 8 + kk % 8)
                           : idx;
    bt_hi[o] = (uint16_t)(pk >> 16);
    bt_lo[o] = (uint16_t)(pk & 0xffffu);
  }
}


// ---- Backward's dense products in one launch (common.h: DenseShare) --------------------------------------------------------
// A role's kind: family | output mode << 4 | width (strip: k-steps; NN: 64-column blocks; TN: the format of the A rows).
// Only the buffer-load forms with 64-column workgroups take part (gemm_*_sharable): the T16 rows and the guarded-load forms
// keep their own launches, and so do the 128-column NN forms -- at 260-268 registers they would hold every role of the
// launch to one workgroup per CU, where the forms below leave two (profiles/bwd_dense_shared.txt).
constexpr int kRoleStrip = 1 << 8, kRoleNnWords = 2 << 8, kRoleNnT24 = 3 << 8, kRoleTn = 4 << 8;
constexpr int dense_role_kind(int family, int mode, int width) { return family | mode << 4 | width; }

// The bodies of the kernels above on a role's virtual index and on LDS images carved from the launch's dynamic LDS (every
// role's images start at its first byte: a workgroup costs the largest role's LDS, not their sum).  The locals carry the names
// of the kernels' parameters: the included texts read them.
// the dynamic LDS of the launch (every declaration of an unsized shared array names its first byte)
__device__ __forceinline__ char* dynamic_lds() {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  return smem;
}
#undef SE3_GRID_BLOCK
#define SE3_GRID_BLOCK vblock
template <int OUT_MODE, int NB>
__device__ __forceinline__ void dense_role_nn_words(const VirtGrid vblock, const DenseRole& r) {
  constexpr bool FAST = true;
  constexpr int BNW = BN * NB;
  char* const lds = dynamic_lds();
  auto as = reinterpret_cast<uint32_t(*)[BM][A_LD]>(lds);
  auto bsh = reinterpret_cast<uint16_t(*)[BNW][B_LD]>(lds + gemm_nn_bf16_lds_bytes(0));
  auto bsl = reinterpret_cast<uint16_t(*)[BNW][B_LD]>(lds + gemm_nn_bf16_lds_bytes(0) + 2 * BNW * B_LD * 2);
  const uint32_t* __restrict__ a = static_cast<const uint32_t*>(r.a);
  const uint16_t* __restrict__ bt_hi = static_cast<const uint16_t*>(r.b0);
  const uint16_t* __restrict__ bt_lo = static_cast<const uint16_t*>(r.b1);
  void* __restrict__ c = r.c;
  const int64_t m = r.m;
  const int n = r.n, k = r.k, kp = r.kp, kt_per_split = r.per;
  const float* __restrict__ alpha_num = r.alpha_num;
  const float alpha_scale = r.alpha_scale;
#include "gemm_nn_bf16_body.h"
}
template <int OUT_MODE, int NB>
__device__ __forceinline__ void dense_role_nn_t24(const VirtGrid vblock, const DenseRole& r) {
  const uint8_t* __restrict__ a = static_cast<const uint8_t*>(r.a);
  const uint16_t* __restrict__ bt_hi = static_cast<const uint16_t*>(r.b0);
  const uint16_t* __restrict__ bt_lo = static_cast<const uint16_t*>(r.b1);
  void* __restrict__ c = r.c;
  const int64_t m = r.m;
  const int n = r.n, k = r.k, st_per_split = r.per;
  const float* __restrict__ alpha_num = r.alpha_num;
  const float alpha_scale = r.alpha_scale;
#include "gemm_nn_t24_body.h"
}
template <int AFMT>
__device__ __forceinline__ void dense_role_tn(const VirtGrid vblock, const DenseRole& r) {
  constexpr bool FAST = true, A16 = AFMT == 2, A24 = AFMT != 0;
  using L = TnLds<AFMT>;
  char* const lds = dynamic_lds();
  auto at = reinterpret_cast<uint32_t(*)[L::kARows][128]>(lds);
  auto ath = reinterpret_cast<uint16_t(*)[L::kPRows][L::kAPitch]>(lds + L::o_ath);
  auto atl = reinterpret_cast<uint16_t(*)[L::kPRows][L::kAPitch]>(lds + L::o_atl);
  auto bt = reinterpret_cast<uint32_t(*)[L::kARows][BN]>(lds + L::o_bt);
  auto bth = reinterpret_cast<uint16_t(*)[L::kPRows][L::kBPitch]>(lds + L::o_bth);
  auto btl = reinterpret_cast<uint16_t(*)[L::kPRows][L::kBPitch]>(lds + L::o_btl);
  const uint32_t* __restrict__ a = static_cast<const uint32_t*>(r.a);
  const uint32_t* __restrict__ b = static_cast<const uint32_t*>(r.b0);
  float* __restrict__ partials = static_cast<float*>(r.c);
  const int64_t m = r.m, chunk = r.chunk;
  const int ka = r.k, n = r.n;
#include "gemm_tn_bf16_body.h"
}
#undef SE3_GRID_BLOCK
#define SE3_GRID_BLOCK blockIdx

__global__ __launch_bounds__(256) void bwd_dense_shared_kernel(const DenseRoles roles) {
  const unsigned id = blockIdx.x;
  int ri = 0;
  if (roles.count > 1 && id >= roles.role[1].begin) ri = 1;
  if (roles.count > 2 && id >= roles.role[2].begin) ri = 2;
  const DenseRole& r = roles.role[ri];
  const unsigned local = id - r.begin, rest = local / r.gx;
  const VirtGrid g{local % r.gx, rest % r.gy, rest / r.gy, r.gy};
  const auto a = static_cast<const uint32_t*>(r.a);
  const auto b0 = static_cast<const uint16_t*>(r.b0), b1 = static_cast<const uint16_t*>(r.b1);
  switch (r.kind) {
    case dense_role_kind(kRoleStrip, 1, 2): gemm_strip_bf16_body<2>(g, a, b0, b1, static_cast<uint32_t*>(r.c), r.m, r.n, r.k); break;
    case dense_role_kind(kRoleStrip, 1, 4): gemm_strip_bf16_body<4>(g, a, b0, b1, static_cast<uint32_t*>(r.c), r.m, r.n, r.k); break;
    case dense_role_kind(kRoleStrip, 1, 8): gemm_strip_bf16_body<8>(g, a, b0, b1, static_cast<uint32_t*>(r.c), r.m, r.n, r.k); break;
    case dense_role_kind(kRoleNnWords, 0, 1): dense_role_nn_words<0, 1>(g, r); break;
    case dense_role_kind(kRoleNnWords, 1, 1): dense_role_nn_words<1, 1>(g, r); break;
    case dense_role_kind(kRoleNnWords, 2, 1): dense_role_nn_words<2, 1>(g, r); break;
    case dense_role_kind(kRoleNnT24, 0, 1): dense_role_nn_t24<0, 1>(g, r); break;
    case dense_role_kind(kRoleNnT24, 2, 1): dense_role_nn_t24<2, 1>(g, r); break;
    case dense_role_kind(kRoleTn, 2, 0): dense_role_tn<0>(g, r); break;
    case dense_role_kind(kRoleTn, 2, 1): dense_role_tn<1>(g, r); break;
    default: break;  // (the host adds no other kind)
  }
}

}  // namespace

int launch_prep_weights(const float* w, int c_in, int kb, int c_out, int mode, uint16_t* bt_hi, uint16_t* bt_lo,
                        hipStream_t stream, const float* scale_num, float scale, bool frag_layout) {
  int n, k;
  if (mode == 0) n = c_out, k = c_in * kb;
  else if (mode == 1) n = c_in * kb, k = c_out;
  else if (mode == 2) n = c_in, k = c_out * kb;
  else n = c_out * kb, k = c_in;
  const int kp = (k + 31) / 32 * 32;
  const int64_t total = (int64_t)n * kp;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(prep_weights_kernel, dim3(blocks), dim3(256), 0, stream, w, c_in, kb, c_out, mode, n, k, kp, bt_hi,
                     bt_lo, scale_num, scale, frag_layout ? 1 : 0);
  return check_launch();
}

// Split the k loop over grid.z when the row blocks alone cannot fill the chip (small hierarchy levels):
// a block's k loop is serial, so 64 k-tiles on a handful of blocks would cost ~100 us whatever M is.
// 64-column blocks per workgroup (template NB): 128 columns pay when the k loop is long (T W, U W': k = C*K); for the
// short-k, wide-n products (grad_T beyond the strip kernel's k <= 64) the narrow tile keeps more blocks in flight
int gemm_nn_bf16_col_blocks(int n, int k) { return n > BN && k >= 512 ? 2 : 1; }

int gemm_nn_bf16_splits(int64_t m, int n, int k) {
  const int bnw = BN * gemm_nn_bf16_col_blocks(n, k);
  const int64_t tiles = ((m + BM - 1) / BM) * ((n + bnw - 1) / bnw);
  const int nkt = (k + BK - 1) / BK;
  const int target = 512;  // workgroups aimed at (two per CU); 1024 and 256 measured slower on the 9 k-point level
  if (tiles < 1 || tiles >= target / 2 || nkt < 8) return 1;  // (tiles = 0: an empty cloud)
  // at most `target` workgroups (one more split than fits starts a second, nearly empty round: 144 tiles x 4 splits =
  // 576 on 512 slots took as long as two full rounds), at least 4 k-tiles per split
  int64_t s_max = target / tiles;
  if (s_max > nkt / 4) s_max = nkt / 4;
  if (s_max < 1) s_max = 1;
  // Cost model in microseconds, fitted to the stage times of the small and mid-sized levels (profiles/r03_nn_split_sweep.txt:
  // forced split counts on the 18 k-row headline level and the 4 k-row / 128-channel DFaust level): a block's k loop is
  // serial at ~0.75 us per 32-k tile (1.1 us with 128-column tiles); the A stream (~3.5 bytes per element) runs at the
  // rate of the level it comes from -- rows of up to ~200 MB were written by the kernel in front and are still in the
  // memory-side cache (9 TB/s), larger ones come from HBM (4.5 TB/s) -- times the share of the 512 workgroup slots that
  // are filled; a split costs its reduction launch (~12 us with the gap in front of it) and the partials written and
  // read back (~0.5 us per MB and split).  64 splits of a 512 x 256 output spent more on 33 MB of partials than on the
  // GEMM; 2 or 4 instead of 3 splits of the 18 k-row level cost 10 us each way.
  const double a_bytes = (double)m * k * 3.5, out_bytes = (double)m * n * 4.0;
  const double t_tile = bnw > BN ? 1.1 : 0.75, rate = a_bytes <= 200e6 ? 9.0e6 : 4.5e6;
  int best = 1;
  double best_cost = 1e30;
  for (int64_t s = 1; s <= s_max; ++s) {
    const int per = (int)((nkt + s - 1) / s);
    const int s_eff = (nkt + per - 1) / per;
    const double fill = (double)(tiles * s_eff) / (double)target;
    const double t_loop = per * t_tile, t_stream = a_bytes / (rate * (fill < 1.0 ? fill : 1.0));
    const double cost = (t_loop > t_stream ? t_loop : t_stream) + (s_eff > 1 ? 12.0 + s_eff * out_bytes * 0.5e-6 : 0.0);
    if (cost < best_cost) best_cost = cost, best = s_eff;
  }
  return best;
}

// Row-strip kernel: packed output, k <= 64, n a multiple of 32, weights prepared with frag_layout and alpha folded in.
bool gemm_strip_bf16_applicable(int64_t m, int n, int k) {
  const int kp = (k + 31) / 32 * 32;
  return kp <= 128 && kp != 96 && n >= 512 && n % 32 == 0 && n <= (1 << 22) && m >= 128 * 16 &&
         (m + 128) * (int64_t)k * 4 < (1ll << 32) - 64 && (int64_t)(n + 64) * kp * 2 < (1ll << 32) - 64;
}

// k-steps of 16 per row of the strip kernel (its template argument) and its grid
struct GemmStripForm { int ks; dim3 grid; };
static GemmStripForm gemm_strip_bf16_form(int64_t m, int n, int k) {
  const int64_t row_blocks = (m + 127) / 128;
  int n_split = row_blocks >= 1024 ? 1 : (int)(1024 / row_blocks);  // <= 1024 workgroups = one resident round (4 per CU)
  const int n_tiles = n / 32;
  if (n_split > n_tiles / 4) n_split = n_tiles / 4 > 0 ? n_tiles / 4 : 1;  // >= 4 column tiles per block
  const int kp = (k + 31) / 32 * 32;
  return {kp == 32 ? 2 : kp == 64 ? 4 : 8, dim3((unsigned)row_blocks, (unsigned)n_split)};
}

// A kernel whose dynamic LDS exceeds the default limit of 64 KB: the limit is raised once per (device, instantiation) -- a
// runtime that keeps the attribute per device must see it on every device the process uses; `raised` is the instantiation's
// set of devices done.  A failure is not cached.
static int raise_dynamic_lds(const void* kernel, int bytes, std::atomic<uint64_t>& raised) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return SE3_ERR_LAUNCH;
  const uint64_t bit = 1ull << (dev & 63);
  if (raised.load(std::memory_order_relaxed) & bit) return SE3_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return SE3_ERR_LAUNCH;
  raised.fetch_or(bit, std::memory_order_relaxed);
  return SE3_OK;
}

// ---- DenseShare: the roles of a shared launch ------------------------------------------------------------------------------
int DenseShare::add(const DenseRole& r, dim3 grid, int lds) {
  if (roles.count >= 3 || (int64_t)grid.x * grid.y * grid.z >= (1ll << 30)) return SE3_ERR_UNSUPPORTED;
  int at = roles.count;
  while (at > 0 && order[at - 1] > next_order) roles.role[at] = roles.role[at - 1], order[at] = order[at - 1], --at;
  roles.role[at] = r;
  roles.role[at].gx = grid.x, roles.role[at].gy = grid.y, roles.role[at].gz = grid.z;
  order[at] = next_order;
  ++roles.count;
  if (lds > lds_bytes) lds_bytes = lds;
  return SE3_OK;
}

constexpr int kDenseSharedMaxLds = TnLds<1>::bytes;  // the widest role: 65.5 KB (NN over packed words: 56 KB, over 3-byte rows: 52 KB, TN over words: 50 KB)
static_assert(kDenseSharedMaxLds >= gemm_nn_bf16_lds_bytes(1) && kDenseSharedMaxLds >= gemm_nn_t24_lds_bytes(1) && kDenseSharedMaxLds >= TnLds<0>::bytes, "");

int DenseShare::launch(hipStream_t stream) {
  if (forms_only()) return form_report("bwd_dense_shared", "one_launch");
  if (roles.count == 0) return SE3_OK;
  unsigned blocks = 0;
  for (int i = 0; i < roles.count; ++i) {
    DenseRole& r = roles.role[i];
    r.begin = blocks;
    blocks += r.gx * r.gy * r.gz;
  }
  {
    ProfScope prof("bwd_dense_shared", stream);
    static std::atomic<uint64_t> raised;
    if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(bwd_dense_shared_kernel), kDenseSharedMaxLds, raised)) return rc;
    hipLaunchKernelGGL(bwd_dense_shared_kernel, dim3(blocks), dim3(256), lds_bytes, stream, roles);
  }
  if (after.set) {
    const int rb = (int)((after.count + 255) / 256 < 2048 ? (after.count + 255) / 256 : 2048);
    if (after.packed)
      hipLaunchKernelGGL(reduce_splits_kernel<true>, dim3(rb), dim3(256), 0, stream, after.partials, after.out, after.count,
                         after.splits, after.alpha_num, after.alpha_scale);
    else
      hipLaunchKernelGGL(reduce_splits_kernel<false>, dim3(rb), dim3(256), 0, stream, after.partials, after.out, after.count,
                         after.splits, after.alpha_num, after.alpha_scale);
  }
  return check_launch();
}

int launch_gemm_strip_bf16(const char* tag, const uint32_t* a, const uint16_t* bt_hi, const uint16_t* bt_lo, uint32_t* c,
                           int64_t m, int n, int k, hipStream_t stream, DenseShare* share) {
  if (m == 0 || n == 0) return SE3_OK;
  if (!gemm_strip_bf16_applicable(m, n, k)) return SE3_ERR_UNSUPPORTED;
  const GemmStripForm f = gemm_strip_bf16_form(m, n, k);
  if (forms_only()) return form_report(tag, "gemm_strip_bf16<ks=%d>", f.ks);
  ProfScope prof(tag, stream);  // (a role of a shared launch keeps its stage's launch count; its time is the shared launch's)
  if (share) {
    DenseRole r{};
    r.kind = dense_role_kind(kRoleStrip, 1, f.ks);
    r.a = a, r.b0 = bt_hi, r.b1 = bt_lo, r.c = c, r.m = m, r.n = n, r.k = k;
    return share->add(r, f.grid, 0);
  }
  const auto kernel = f.ks == 2 ? gemm_strip_bf16_kernel<2> : f.ks == 4 ? gemm_strip_bf16_kernel<4> : gemm_strip_bf16_kernel<8>;
  hipLaunchKernelGGL(kernel, f.grid, dim3(256), 0, stream, a, bt_hi, bt_lo, c, m, n, k);
  return check_launch();
}

// Which NN kernel a block of rows takes (gemm_nn_bf16_rows switches on it): the kernel by the format of the A rows, the
// output mode (0 fp32, 1 packed words, 2 split-K partials), the buffer-load form (`fast`), 64-column blocks per workgroup.
struct GemmNnBf16Form {
  int status;        // SE3_OK, or why the shape cannot run in this row format
  int afmt, mode, nb;
  bool fast;
  int kp, per, st_per, splits;
  dim3 grid;
};
static GemmNnBf16Form gemm_nn_bf16_form(int64_t m, int n, int k, bool have_split_ws, bool out_packed, int afmt) {
  GemmNnBf16Form f{};
  const bool a24 = afmt == 1, a16 = afmt == 2;  // A rows: 0 packed words, 1 3-byte rows, 2 T16 (common.h)
  f.afmt = afmt;
  f.kp = (k + 31) / 32 * 32;
  const int nkt = f.kp / BK;
  int splits = have_split_ws ? gemm_nn_bf16_splits(m, n, k) : 1;
  f.per = (nkt + splits - 1) / splits;
  splits = (nkt + f.per - 1) / f.per;
  f.nb = gemm_nn_bf16_col_blocks(n, k);
  f.grid = dim3((unsigned)((m + BM - 1) / BM), (unsigned)((n + BN * f.nb - 1) / (BN * f.nb)), (unsigned)splits);
  f.fast = (k % 32 == 0) && (m * (int64_t)k * 4 < (1ll << 32)) && ((int64_t)n * f.kp * 2 < (1ll << 32)) &&
           ((m + BM) * (int64_t)k * 4 < (1ll << 32)) && ((int64_t)(n + 128) * f.kp * 2 < (1ll << 32));
  if (a24 && (!f.fast || k % 64 != 0)) f.status = SE3_ERR_UNSUPPORTED;
  // T16: mega tiles of 256 k; its rows are 2.25 bytes per element, addressed with 32-bit byte offsets like the others
  if (a16 && (k % 256 != 0 || (m + BM) * gemm_a_row_bytes(afmt, k) >= (1ll << 32) || (int64_t)(n + 128) * f.kp * 2 >= (1ll << 32)))
    f.status = SE3_ERR_UNSUPPORTED;
  if (f.status) return f;
  f.st_per = (f.per + 1) / 2;  // 3-byte / T16 rows: the kernels walk super tiles of 64 k
  if (a16) f.st_per = (f.st_per + 3) / 4 * 4;  // whole mega tiles per split
  if (a24 || a16) {
    splits = (k / 64 + f.st_per - 1) / f.st_per;
    f.grid.z = (unsigned)splits;
  }
  f.splits = splits;
  f.mode = splits > 1 ? 2 : out_packed ? 1 : 0;
  return f;
}

// The NN kernel of a form, by (output mode; row format; `fast`, 64-column blocks per workgroup - 1)
using NnWordsKernel = void (*)(const uint32_t*, const uint16_t*, const uint16_t*, void*, int64_t, int, int, int, int, const float*, float);
using NnPlanesKernel = void (*)(const uint8_t*, const uint16_t*, const uint16_t*, void*, int64_t, int, int, int, const float*, float);
struct NnKernels { NnWordsKernel words[2][2]; NnPlanesKernel t24[2], t16[2]; };
template <int MODE>
static constexpr NnKernels nn_kernels() {
  return {{{gemm_nn_bf16_kernel<MODE, false, 1>, gemm_nn_bf16_kernel<MODE, false, 2>},
           {gemm_nn_bf16_kernel<MODE, true, 1>, gemm_nn_bf16_kernel<MODE, true, 2>}},
          {gemm_nn_t24_kernel<MODE, 1>, gemm_nn_t24_kernel<MODE, 2>},
          {gemm_nn_t16_kernel<MODE, 1>, gemm_nn_t16_kernel<MODE, 2>}};
}
static const NnKernels kNnKernels[3] = {nn_kernels<0>(), nn_kernels<1>(), nn_kernels<2>()};

static int gemm_nn_bf16_rows(const char* tag, const uint32_t* a, const uint16_t* bt_hi, const uint16_t* bt_lo, void* c,
                             bool out_packed, int64_t m, int n, int k, float* split_ws, const float* alpha_num, float alpha_scale,
                             hipStream_t stream, int afmt, ReduceBatch* defer, DenseShare* share) {
  const GemmNnBf16Form f = gemm_nn_bf16_form(m, n, k, split_ws != nullptr, out_packed, afmt);
  if (f.status) return f.status;
  const int kp = f.kp, per = f.per, st_per = f.st_per, splits = f.splits;
  const dim3 grid = f.grid;
  void* const out = f.mode == 2 ? (void*)split_ws : c;
  if (forms_only()) {
    if (afmt == 0) form_report(tag, "gemm_nn_bf16<mode=%d,fast=%d,nb=%d>", f.mode, f.fast, f.nb);
    else form_report(tag, "gemm_nn_%s<mode=%d,nb=%d>", afmt == 2 ? "t16" : "t24", f.mode, f.nb);
    if (splits > 1 && !defer) form_report(tag, "reduce_splits<packed=%d>", out_packed);
  } else {
    const bool planes = f.afmt == 1 || f.afmt == 2;
    if (f.mode < 0 || f.mode > 2 || f.nb < 1 || f.nb > 2 || (f.afmt != 0 && !planes)) return SE3_ERR_UNSUPPORTED;
    const NnKernels& ks = kNnKernels[f.mode];
    if (share) {  // a role of the caller's shared launch: the buffer-load forms over packed words and 3-byte rows
      if (f.afmt == 2 || (f.afmt == 0 && !f.fast) || f.nb != 1) return SE3_ERR_UNSUPPORTED;
      DenseRole r{};
      r.kind = dense_role_kind(planes ? kRoleNnT24 : kRoleNnWords, f.mode, f.nb);
      r.a = a, r.b0 = bt_hi, r.b1 = bt_lo, r.c = out, r.m = m, r.n = n, r.k = k, r.kp = kp, r.per = planes ? st_per : per;
      r.alpha_num = alpha_num, r.alpha_scale = alpha_scale;
      if (int rc = share->add(r, grid, planes ? gemm_nn_t24_lds_bytes(f.nb) : gemm_nn_bf16_lds_bytes(f.nb))) return rc;
    } else if (planes) {
      const NnPlanesKernel kernel = f.afmt == 1 ? ks.t24[f.nb - 1] : ks.t16[f.nb - 1];
      const int lds_bytes = f.afmt == 1 ? gemm_nn_t24_lds_bytes(f.nb) : 0;  // t16: static LDS
      // per t24 instantiation [mode][nb - 1]: the devices whose limit has been raised (only nb = 2, 72 KB, is beyond the default)
      static std::atomic<uint64_t> raised[3][2];
      if (lds_bytes > 64 * 1024)
        if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_bytes, raised[f.mode][f.nb - 1])) return rc;
      hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, stream, (const uint8_t*)a, bt_hi, bt_lo, out, m, n, k, st_per,
                         alpha_num, alpha_scale);
    } else {
      hipLaunchKernelGGL(ks.words[f.fast][f.nb - 1], grid, dim3(256), 0, stream, a, bt_hi, bt_lo, out, m, n, k, kp, per,
                         alpha_num, alpha_scale);
    }
  }
  if (splits > 1) {
    const int64_t count = m * n;
    const int rb = (int)((count + 255) / 256 < 2048 ? (count + 255) / 256 : 2048);
    if (defer)  // the caller folds the partials together with its other reductions (ReduceBatch)
      defer->sum(split_ws, c, count, splits, alpha_num, alpha_scale, out_packed);
    else if (forms_only())
      ;
    else if (share)  // behind the shared launch
      share->after = {split_ws, c, count, splits, alpha_num, alpha_scale, out_packed, true};
    else if (out_packed)
      hipLaunchKernelGGL(reduce_splits_kernel<true>, dim3(rb), dim3(256), 0, stream, split_ws, c, count, splits,
                         alpha_num, alpha_scale);
    else
      hipLaunchKernelGGL(reduce_splits_kernel<false>, dim3(rb), dim3(256), 0, stream, split_ws, c, count, splits,
                         alpha_num, alpha_scale);
  }
  return check_launch();
}

// The kernels address A with 32-bit byte offsets (buffer loads): more rows than those reach -- 262 k rows of 2048 values
// and up, i.e. clouds beyond ~130 k points at two frames -- go through the same kernels row block by row block (no split
// of k at that size, so the blocks share nothing but the weights).  0: the whole product is one block.
static int64_t gemm_nn_bf16_row_block(int64_t m, int k) {
  const int64_t max_rows = (((1ll << 32) - 64) / ((int64_t)k * 4) - 2 * BM) / BM * BM;
  return m <= max_rows || max_rows < BM || k % 32 != 0 ? 0 : max_rows;
}

int launch_gemm_nn_bf16(const char* tag, const uint32_t* a, const uint16_t* bt_hi, const uint16_t* bt_lo, void* c,
                        bool out_packed, int64_t m, int n, int k, float* split_ws, const float* alpha_num,
                        float alpha_scale, hipStream_t stream, int afmt, ReduceBatch* defer, DenseShare* share) {
  if (m == 0 || n == 0) return SE3_OK;
  const int64_t max_rows = gemm_nn_bf16_row_block(m, k);
  if (share && max_rows) return SE3_ERR_UNSUPPORTED;  // (gemm_nn_bf16_sharable)
  if (forms_only() && max_rows) form_report(tag, "gemm_nn_row_blocks");
  ProfScope prof(tag, stream);
  if (!max_rows)
    return gemm_nn_bf16_rows(tag, a, bt_hi, bt_lo, c, out_packed, m, n, k, split_ws, alpha_num, alpha_scale, stream, afmt, defer, share);
  const int64_t a_row_bytes = gemm_a_row_bytes(afmt, k);
  for (int64_t m0 = 0; m0 < m; m0 += max_rows) {
    const int64_t mb = m - m0 < max_rows ? m - m0 : max_rows;
    if (int rc = gemm_nn_bf16_rows(tag, reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a) + m0 * a_row_bytes), bt_hi,
                                   bt_lo, static_cast<char*>(c) + m0 * (int64_t)n * 4, out_packed, mb, n, k, nullptr, alpha_num,
                                   alpha_scale, stream, afmt, nullptr, nullptr))
      return rc;
  }
  return SE3_OK;
}

// Whether the product can be a role of a shared launch: one block of rows, a buffer-load form with 64-column workgroups, no T16 rows
bool gemm_nn_bf16_sharable(int64_t m, int n, int k, bool out_packed, int afmt) {
  if (m <= 0 || n <= 0 || gemm_nn_bf16_row_block(m, k)) return false;
  const GemmNnBf16Form f = gemm_nn_bf16_form(m, n, k, true, out_packed, afmt);
  return !f.status && f.afmt != 2 && (f.afmt == 1 || f.fast) && f.nb == 1;
}

size_t gemm_nn_bf16_split_bytes(int64_t m, int n, int k) {
  const int s = gemm_nn_bf16_splits(m, n, k);
  return s > 1 ? (size_t)s * m * n * 4 : 0;
}

// Which TN kernel a weight-gradient product takes: by the format of the A rows; packed-word rows take the buffer-load
// form (`fast`) when n is a multiple of 4 and a launch's 32-bit offsets reach a range plus its prefetch
struct GemmTnBf16Form { int status; bool fast; int afmt; int64_t chunk, zs; };
static GemmTnBf16Form gemm_tn_bf16_form(int64_t m, int ka, int n, int splits, int afmt) {
  GemmTnBf16Form f{};
  const bool a24 = afmt == 1, a16 = afmt == 2;
  f.afmt = afmt;
  f.chunk = (m + splits - 1) / splits;
  f.chunk = (f.chunk + BK - 1) / BK * BK;
  if (f.chunk == 0) f.chunk = BK;
  // Both operands are addressed with 32-bit byte offsets from the pointers the kernel gets: row ranges (grid.z) beyond
  // their reach are launched as further groups of ranges, each with its operands' pointers moved to its first row
  // (the partials of group j start at range j * zs of the same buffer).
  const int64_t widest = (int64_t)(ka > n ? ka : n) * 4;
  f.zs = (((1ll << 32) - 64) / widest - f.chunk) / f.chunk;  // ranges one launch can address
  if (f.zs < 1) f.zs = 1;
  if (f.zs > splits) f.zs = splits;
  const bool vec = n % 4 == 0, reach = (f.zs + 1) * f.chunk * widest < (1ll << 32) - 64;
  if (a24 && (!vec || !reach || ka % 64 != 0)) f.status = SE3_ERR_UNSUPPORTED;
  if (a16 && (!vec || !reach || ka % 256 != 0)) f.status = SE3_ERR_UNSUPPORTED;
  f.fast = a16 || a24 || (vec && reach);
  return f;
}

bool gemm_tn_bf16_sharable(int64_t m, int ka, int n, int splits, int afmt) {
  if (m <= 0 || ka <= 0 || n <= 0 || splits < 1) return false;
  const GemmTnBf16Form f = gemm_tn_bf16_form(m, ka, n, splits, afmt);
  return !f.status && f.fast && f.afmt != 2 && f.zs >= splits;
}

int launch_gemm_tn_bf16(const char* tag, const uint32_t* a, const uint32_t* b, float* c, float* partials, int splits,
                        int64_t m, int ka, int n, const float* alpha_num, float alpha_scale, hipStream_t stream, int afmt,
                        ReduceBatch* defer, bool out_ikn, DenseShare* share) {
  if (ka == 0 || n == 0) return SE3_OK;
  if (out_ikn && (!defer || ka % kBasis != 0)) return SE3_ERR_INVALID_ARGUMENT;  // the permuted store lives in the batched reduction
  const GemmTnBf16Form f = gemm_tn_bf16_form(m, ka, n, splits, afmt);
  if (f.status) return f.status;
  if (forms_only()) {
    form_report(tag, "gemm_tn_bf16<fast=%d,afmt=%d>", f.fast, f.afmt);
    if (defer) {
      defer->sum(partials, c, (int64_t)ka * n, splits, alpha_num, alpha_scale, false, out_ikn ? n : 0);
      return SE3_OK;
    }
    return launch_reduce_partials(partials, c, (int64_t)ka * n, splits, alpha_num, alpha_scale, stream);
  }
  ProfScope prof(tag, stream);
  const int64_t chunk = f.chunk, zs = f.zs;
  if (share) {  // a role of the caller's shared launch: every row range in one grid, a buffer-load form (gemm_tn_bf16_sharable)
    if (!f.fast || f.afmt == 2 || zs < splits || m <= 0 || !defer) return SE3_ERR_UNSUPPORTED;
    DenseRole r{};
    r.kind = dense_role_kind(kRoleTn, 2, f.afmt);
    r.a = a, r.b0 = b, r.c = partials, r.m = m, r.chunk = chunk, r.n = n, r.k = ka;
    if (int rc = share->add(r, dim3((unsigned)((ka + 127) / 128), (unsigned)((n + BN - 1) / BN), (unsigned)splits),
                            f.afmt == 1 ? TnLds<1>::bytes : TnLds<0>::bytes))
      return rc;
    defer->sum(partials, c, (int64_t)ka * n, splits, alpha_num, alpha_scale, false, out_ikn ? n : 0);
    return SE3_OK;
  }
  const auto kernel = !f.fast      ? gemm_tn_bf16_kernel<false, 0>
                      : f.afmt == 2 ? gemm_tn_bf16_kernel<true, 2>
                      : f.afmt == 1 ? gemm_tn_bf16_kernel<true, 1>
                                    : gemm_tn_bf16_kernel<true, 0>;
  for (int64_t z0 = 0; z0 < splits; z0 += zs) {
    const int64_t zn = splits - z0 < zs ? splits - z0 : zs, r0 = z0 * chunk;
    if (r0 >= m) {  // ranges past the last row (rounding of chunk): their partials are zeros
      if (int rc = launch_fill_words(partials + z0 * ka * n, 0u, (int64_t)(splits - z0) * ka * n, stream)) return rc;
      break;
    }
    const int64_t mb = m - r0 < zn * chunk ? m - r0 : zn * chunk;
    const dim3 grid((unsigned)((ka + 127) / 128), (unsigned)((n + BN - 1) / BN), (unsigned)zn);
    const uint32_t* ab = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a) + r0 * gemm_a_row_bytes(afmt, ka));
    const uint32_t* bb = b + r0 * n;
    float* pb = partials + z0 * ka * n;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, ab, bb, pb, mb, ka, n, chunk);
  }
  if (defer) {
    defer->sum(partials, c, (int64_t)ka * n, splits, alpha_num, alpha_scale, false, out_ikn ? n : 0);
    return check_launch();
  }
  return launch_reduce_partials(partials, c, (int64_t)ka * n, splits, alpha_num, alpha_scale, stream);
}

}  // namespace se3
