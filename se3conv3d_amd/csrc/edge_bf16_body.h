// The pieces of a 32-frame-edge chunk that the four forms of the split-bf16 edge pass (edge_bf16.hip) are made of, each
// defined once: the feature-word gather, GELU + hi/lo split of a k-step, the wave-pair chunk (MLP | publish | aggregate),
// the single-wavefront chunk, the 3-byte row store, the cursor of the chunk-stream kernels -- and the per-item body of the
// single-wavefront kernel, which (like the one-item wave-pair kernel) takes gelu_frags and t24_store2 only and keeps its own
// text of the rest.  edge_dx.hip takes the GELU + split and MlpOperand.  See edge_bf16.hip for the scheme.
#pragma once

#include "common.h"

namespace se3 {

// MLP weights [A; beta] as MFMA B fragments in LDS: arrangement a has descriptor dims 0..7 in the lane
// half that builds row a's descriptors.  Called by the first wavefront of a block.
template <int FC>
__device__ __forceinline__ void mlp_weights_to_lds(uint32_t (*lds_w)[2][64][4], const float* __restrict__ axes_ext,
                                                   int lane) {
  const int kcol = lane & 31, h = lane >> 5;
  float v07[8], v89[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v07[j] = kGeluIn * axes_ext[j * kBasis + kcol];  // the MLP delivers kGeluIn * pre (gelu_scaled)
    v89[j] = j < 2 ? kGeluIn * axes_ext[(8 + j) * kBasis + kcol] : 0.f;
  }
#pragma unroll
  for (int a = 0; a < FC; ++a) {
    const bool dims07 = FC == 1 ? h == 0 : h == a;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = dims07 ? v07[j] : v89[j];
    u32x4 w_hi, w_lo;
    frags_from_floats(v, w_hi, w_lo);
    *reinterpret_cast<u32x4*>(&lds_w[a][0][lane][0]) = w_hi;
    *reinterpret_cast<u32x4*>(&lds_w[a][1][lane][0]) = w_lo;
  }
}

// ------------------------------------------------------------------------------------------------
// Pieces of a chunk
// ------------------------------------------------------------------------------------------------
// Gathered feature words of a chunk's two k-steps.  The byte offset of the source row of frame-edge acc_row(8s + j, h) (qoff
// of the lane that owns it) comes by ds_bpermute; from it the lane loads either one piece of VW words at byte cb4[0]
// (fw[s][i][j] = word i) or one word for each of NT tiles at bytes cb4[t] (fw[s][t][j]).
// All loads go out at once; a tile that is not ch_ok, and rows past the end of the list, read out of bounds (0).
// (no branch around the second k-step's loads: a conditional load makes every counted s_waitcnt behind it assume the loads
// were not issued, i.e. wait for all of them)
template <int VW, int NT>
__device__ __forceinline__ void gather_feature_words(const __amdgpu_buffer_rsrc_t feat_rs, int hb, int qoff,
                                                     const int (&cb4)[NT], const bool (&ch_ok)[NT],
                                                     uint32_t (&fw)[2][NT * VW][8]) {
  static_assert(VW == 1 || NT == 1, "one wide piece or NT single words");
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int src_off = __builtin_amdgcn_ds_bpermute(hb + 4 * acc_row(8 * s + j, 0), qoff);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int voff = ch_ok[t] ? src_off + cb4[t] : kOobOffset;
        if constexpr (VW == 4) {
          const auto v = __builtin_amdgcn_raw_buffer_load_b128(feat_rs, voff, 0, 0);
          fw[s][0][j] = v[0], fw[s][1][j] = v[1], fw[s][2][j] = v[2], fw[s][3][j] = v[3];
        } else if constexpr (VW == 2) {
          const auto v = __builtin_amdgcn_raw_buffer_load_b64(feat_rs, voff, 0, 0);
          fw[s][0][j] = v[0], fw[s][1][j] = v[1];
        } else {
          fw[s][t][j] = __builtin_amdgcn_raw_buffer_load_b32(feat_rs, voff, 0, 0);
        }
      }
    }
  }
}

// GELU of k-step s of an MLP result (its accumulator registers 8s .. 8s + 7) as hi / lo MFMA fragments
__device__ __forceinline__ void gelu_frags(const f32x16& phi, int s, u32x4& hi, u32x4& lo) {
  float pv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) pv[j] = gelu_scaled(phi[8 * s + j]);
  frags_from_floats(pv, hi, lo);
}

// Wave-pair chunk, in the three pieces between which the kernels put their barrier (and the timeline build its stamps).
// Kernel MLP of this wavefront's frame; both lane halves hold the same descriptor: half 0 feeds dims 0..7, half 1 dims 8, 9
__device__ __forceinline__ f32x16 pair_mlp(const float d[9], int lane, const uint32_t (*lds_w)[2][64][4]) {
  const int h = lane >> 5;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = h ? (j == 0 ? d[8] : (j == 1 ? 1.0f : 0.f)) : d[j];
  u32x4 a_hi, a_lo;
  frags_from_floats(v, a_hi, a_lo);
  const u32x4 wb_hi = *reinterpret_cast<const u32x4*>(&lds_w[0][0][lane][0]);
  const u32x4 wb_lo = *reinterpret_cast<const u32x4*>(&lds_w[0][1][lane][0]);
  return mfma_bf16x3(a_hi, a_lo, wb_hi, wb_lo, zero16());
}
// GELU + split of phi into phi_buf[frame][k-step][hi/lo][lane].  NF = 2: wavefront wv owns frame wv; NF = 1: one frame,
// wavefront wv does k-step wv only.
template <int NF>
__device__ __forceinline__ void pair_publish(const f32x16& phi, int cnt, int wv, int lane, uint32_t (*phi_buf)[2][2][64][4]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s * 16 < cnt && (NF == 2 || s == wv)) {
      u32x4 b_hi, b_lo;
      gelu_frags(phi, s, b_hi, b_lo);
      *reinterpret_cast<u32x4*>(&phi_buf[NF == 2 ? wv : 0][s][0][lane][0]) = b_hi;
      *reinterpret_cast<u32x4*>(&phi_buf[NF == 2 ? wv : 0][s][1][lane][0]) = b_lo;
    }
  }
}
// acc[a][t] += (feature words of tile t)^T phi of frame a -- behind the barrier that follows pair_publish
template <int CT, int NF>
__device__ __forceinline__ void pair_aggregate(const uint32_t (*phi_buf)[2][2][64][4], int cnt, int lane,
                                               const uint32_t (&fw)[2][CT][8], f32x16 (&acc)[NF][CT]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s * 16 < cnt) {
      u32x4 b_hi[NF], b_lo[NF];
#pragma unroll
      for (int a = 0; a < NF; ++a) {
        b_hi[a] = *reinterpret_cast<const u32x4*>(&phi_buf[a][s][0][lane][0]);
        b_lo[a] = *reinterpret_cast<const u32x4*>(&phi_buf[a][s][1][lane][0]);
      }
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        u32x4 fa_hi, fa_lo;
        frags_from_words(fw[s][t], fa_hi, fa_lo);
#pragma unroll
        for (int a = 0; a < NF; ++a) acc[a][t] = mfma_bf16x3(fa_hi, fa_lo, b_hi[a], b_lo[a], acc[a][t]);
      }
    }
  }
}

// Single-wavefront chunk.  With FC = 2 lanes of half h hold the descriptor against frame a0 + h; row a's dims 8, 9 live in
// half 1 - a.  The MLP A operand pieces of this lane: its own dims 0..7, and {dim 8 of the row it serves as "other" half, 1}
template <int FC>
struct MlpOperand {
  u32x4 own_hi, own_lo, oth_hi, oth_lo;
  __device__ __forceinline__ MlpOperand(const float d[9], int h) {
    frags_from_floats(d, own_hi, own_lo);
    float d8 = d[8];
    if constexpr (FC == 2) {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(d8), __float_as_uint(d8), false, false);
      d8 = __uint_as_float(h ? sw[0] : sw[1]);
    }
    uint32_t p_hi, p_lo;
    split2(d8, 1.0f, p_hi, p_lo);
    oth_hi = u32x4{p_hi, 0u, 0u, 0u};
    oth_lo = u32x4{p_lo, 0u, 0u, 0u};
  }
};
// Frame a of the chunk: phi of the frame, GELU, acc[t] += (feature words of tile t)^T phi.  The first frame turns the
// words into fragments at their first use (they have had a chunk's work to arrive), the second finds them in fa.
template <int VW, int FC>
__device__ __forceinline__ void single_frame(int a, const MlpOperand<FC>& op, int cnt, int lane,
                                             const uint32_t (*lds_w)[2][64][4], const uint32_t (&fw)[2][VW][8],
                                             u32x4 (&fa_hi)[2][VW], u32x4 (&fa_lo)[2][VW], f32x16 (&acc)[VW]) {
  const bool dims07 = FC == 1 ? (lane >> 5) == 0 : (lane >> 5) == a;
  u32x4 a_hi, a_lo;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a_hi[i] = dims07 ? op.own_hi[i] : op.oth_hi[i];
    a_lo[i] = dims07 ? op.own_lo[i] : op.oth_lo[i];
  }
  const u32x4 wb_hi = *reinterpret_cast<const u32x4*>(&lds_w[a][0][lane][0]);
  const u32x4 wb_lo = *reinterpret_cast<const u32x4*>(&lds_w[a][1][lane][0]);
  const f32x16 phi = mfma_bf16x3(a_hi, a_lo, wb_hi, wb_lo, zero16());
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s * 16 < cnt) {
      u32x4 b_hi, b_lo;
      gelu_frags(phi, s, b_hi, b_lo);
#pragma unroll
      for (int t = 0; t < VW; ++t) {
        if (a == 0) frags_from_words(fw[s][t], fa_hi[s][t], fa_lo[s][t]);
        acc[t] = mfma_bf16x3(fa_hi[s][t], fa_lo[s][t], b_hi, b_lo, acc[t]);
      }
    }
  }
}

// 3-byte rows (common.h): channels ch0 (even), ch0 + 1 of basis function kcol = one hi word + one lo half-word, non-temporal
__device__ __forceinline__ void t24_store2(char* row, int C, int ch0, int kcol, float x0, float x1) {
  uint32_t hp, lp;
  t24_pack2(x0, x1, hp, lp);
  const int idx = (ch0 >> 1) * kBasis + kcol;
  __builtin_nontemporal_store(hp, reinterpret_cast<uint32_t*>(row) + idx);
  __builtin_nontemporal_store((uint16_t)lp, reinterpret_cast<uint16_t*>(row + (int64_t)C * kBasis * 2) + idx);
}
// ... of an accumulator tile: register r of lane (kcol, h) = channel ch_base + acc_row(r, h), registers r, r + 1 adjacent
template <bool FULL>
__device__ __forceinline__ void t24_store_tile(char* row, int C, int ch_base, int h, int kcol, const f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int ch = ch_base + acc_row(r, h);  // even
    if (!FULL && ch >= C) continue;
    t24_store2(row, C, ch, kcol, acc[r], (FULL || ch + 1 < C) ? acc[r + 1] : 0.f);
  }
}

// ------------------------------------------------------------------------------------------------
// Cursor of the chunk-stream kernels: a walker (a wave pair or a wavefront) goes through the chunks of its items
// first, first + stride, ... as one stream, in windows of 64 items whose row extents sit in two registers (lane l = the
// window's l-th item, read with v_readlane: no memory round trip per item).
// ------------------------------------------------------------------------------------------------
struct ChunkCursor {
  int j;        // local item index; n_mine = past the end
  int c0;       // first frame-edge of the chunk
  int start;    // first edge of the item's centre point
  int n_total;  // frame-edges of the item
  int crow;     // the walker's (first) centre row of the item (record index)
  uint32_t item;
};

// (every cursor field is wave-uniform; readfirstlane says so to the compiler: scalar registers, scalar branches)
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

template <int ROWS>  // centre rows (frames) per item
struct ChunkStream {
  const EdgeGeom& g;
  __amdgpu_buffer_rsrc_t nbr_rs;  // g.nbr; ids past the list read 0
  uint32_t first, stride;         // the walker's items
  int n_all;                      // how many of them
  int row_off;                    // the walker's centre row within an item
  int fnb_shift, kcol;
  // the current window
  uint32_t item0;
  int n_mine, v_lo, v_hi;

  __device__ __forceinline__ uint32_t groups() const { return (uint32_t)g.f_ctr / (uint32_t)ROWS; }
  __device__ __forceinline__ void window(int win0, int lane) {
    n_mine = min(64, n_all - win0);
    item0 = first + (uint32_t)win0 * stride;
    const uint32_t item = item0 + (uint32_t)min(lane, n_mine - 1) * stride;
    const uint32_t ctr = item / groups();
    v_hi = g.ends[ctr];
    v_lo = g.ends[max((int)ctr - 1, 0)];
    if (ctr == 0) v_lo = 0;
  }
  __device__ __forceinline__ ChunkCursor enter(int j, int crow_keep, uint32_t item_keep) const {  // first chunk of local item j, or the end mark
    ChunkCursor c;
    c.j = j, c.c0 = 0, c.start = 0, c.n_total = 0;
    c.crow = crow_keep, c.item = item_keep;  // end mark: the last item's record stays the (valid) prefetch target
    if (j < n_mine) {
      const int lo = __builtin_amdgcn_readlane(v_lo, j), hi = __builtin_amdgcn_readlane(v_hi, j);
      c.start = lo, c.n_total = (hi - lo) << fnb_shift;
      c.item = item0 + (uint32_t)j * stride;
      const uint32_t ctr = c.item / groups();
      c.crow = uni((int)(ctr * (uint32_t)g.f_ctr + (c.item - ctr * groups()) * (uint32_t)ROWS) + row_off);
    }
    return c;
  }
  __device__ __forceinline__ ChunkCursor advance(const ChunkCursor& c) const {
    ChunkCursor r = c;
    if (c.c0 + 32 < c.n_total) r.c0 = c.c0 + 32;
    else if (c.j < n_mine) r = enter(c.j + 1, c.crow, c.item);
    r.j = uni(r.j), r.c0 = uni(r.c0), r.start = uni(r.start), r.n_total = uni(r.n_total), r.item = (uint32_t)uni((int)r.item);
    return r;
  }
  // frame-edge of this lane (indices past the end clamp to the last one) -> neighbour id -> source row
  __device__ __forceinline__ int fe_of(const ChunkCursor& c) const { return max(min(c.c0 + kcol, c.n_total - 1), 0); }
  __device__ __forceinline__ int nbr_of(const ChunkCursor& c) const {
    const int e = c.start + (fe_of(c) >> fnb_shift);
    return (int)__builtin_amdgcn_raw_buffer_load_b32(nbr_rs, (e * g.nbr_stride + g.nbr_offset) * 4, 0, 0);
  }
  __device__ __forceinline__ int row_of(int nb, const ChunkCursor& c) const {
    return (nb << fnb_shift) + (fe_of(c) & ((1 << fnb_shift) - 1));
  }
  // Start of a window: its first three chunks, and what the chunk loop carries -- the source rows of this chunk and of the
  // next (ids consumed) and this chunk's record, in flight
  __device__ __forceinline__ void prime(const __amdgpu_buffer_rsrc_t nbg_rs, ChunkCursor& cur, ChunkCursor& n1, ChunkCursor& n2,
                                        int& q_cur, int& q_n1, float xn_nx[3], float rn_nx[9]) const {
    cur = enter(0, 0, 0u);
    n1 = advance(cur);
    n2 = advance(n1);
    const int nb_cur = nbr_of(cur);
    const int nb_n1 = nbr_of(n1);
    q_cur = row_of(nb_cur, cur);
    load_geom_record(nbg_rs, q_cur, xn_nx, rn_nx);
    q_n1 = row_of(nb_n1, n1);
  }
  // The centre record(s) of a chunk are wave-uniform: read through the scalar cache (constant address space + a uniform
  // index = s_load) into SGPRs.  PER_HALF: the record of row crow + h per lane half (selected into registers).
  template <bool PER_HALF>
  __device__ __forceinline__ void centre(const ChunkCursor& c, int h, float yc[3], float rc[9]) const {
    typedef const f32x4 __attribute__((address_space(4))) * crec_t;
    const crec_t ctr_rec = (crec_t)(uintptr_t)g.ctr_geom;
    const int row = c.crow;
    const f32x4 v0 = ctr_rec[row * 4], v1 = ctr_rec[row * 4 + 1], v2 = ctr_rec[row * 4 + 2];
    if constexpr (PER_HALF) {
      const f32x4 w0 = ctr_rec[row * 4 + 4], w1 = ctr_rec[row * 4 + 5], w2 = ctr_rec[row * 4 + 6];
      yc[0] = h ? w0[0] : v0[0], yc[1] = h ? w0[1] : v0[1], yc[2] = h ? w0[2] : v0[2], rc[8] = h ? w0[3] : v0[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) rc[i] = h ? w1[i] : v1[i], rc[4 + i] = h ? w2[i] : v2[i];
    } else {
      yc[0] = v0[0], yc[1] = v0[1], yc[2] = v0[2], rc[8] = v0[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) rc[i] = v1[i], rc[4 + i] = v2[i];
    }
  }
};

// One item = FC frames of one centre point.  sink(a, ch0, ch1, x0, x1, ok0, ok1) receives the values of row
// (ctr*f_ctr + a0 + a), channels ch0 / ch1 (ch1 = ch0 + VW), basis function k = lane & 31, and packs / stores them.
template <int VW, int FC, bool FULL, class Sink>
__device__ __forceinline__ void edge_item_bf16(const EdgeGeom& g, const __amdgpu_buffer_rsrc_t feat_rs, int channels,
                                               const uint32_t (*lds_w)[2][64][4], float rho, int64_t item,
                                               int fnb_shift, Sink&& sink) {
  const int lane = threadIdx.x & 63;
  const int kcol = lane & 31, h = lane >> 5;
  const int groups = g.f_ctr / FC;
  // rows < 2^31 (checked on the host), so 32-bit unsigned division is exact -- the 64-bit one is ~150 scalar instructions
  const int64_t ctr = (uint32_t)item / (uint32_t)groups;
  const int a0 = (int)((uint32_t)item - (uint32_t)ctr * (uint32_t)groups) * FC;

  const int start = ctr > 0 ? g.ends[ctr - 1] : 0;
  const int n_total = (g.ends[ctr] - start) * g.f_nb;
  const __amdgpu_buffer_rsrc_t nbg_rs = buffer_of(g.nb_geom, g.n_nb * g.f_nb * 64);
  float yc[3], rc[9];
  // the centre frame this lane builds descriptors for
  load_geom_record(buffer_of(g.ctr_geom, g.n_ctr * g.f_ctr * 64), (int)(ctr * g.f_ctr + a0 + (FC == 2 ? h : 0)), yc, rc);
  const int row_bytes = channels * 4;
  const int hb = 16 * h;  // ds_bpermute byte address of lane 4h

  for (int cbase = 0; cbase < channels; cbase += 32 * VW) {
    const int cb = cbase + VW * kcol;
    const bool ch_ok[1] = {FULL || cb < channels};
    const int cb4[1] = {(ch_ok[0] ? cb : 0) * 4};
    f32x16 acc[FC][VW];
#pragma unroll
    for (int a = 0; a < FC; ++a)
#pragma unroll
      for (int t = 0; t < VW; ++t) acc[a][t] = zero16();

    // frame-edge -> neighbour id / source row: lane n of both halves handles frame-edge c0 + n (indices past the end
    // clamp to the last one)
    auto nbr_of = [&](int c0) {
      const int fe = min(c0 + kcol, n_total - 1);
      const int e = start + (fnb_shift >= 0 ? fe >> fnb_shift : fe / g.f_nb);
      return g.nbr[(int64_t)e * g.nbr_stride + g.nbr_offset];
    };
    auto row_of = [&](int nb, int c0) {
      const int fe = min(c0 + kcol, n_total - 1);
      return nb * g.f_nb + (fnb_shift >= 0 ? fe & ((1 << fnb_shift) - 1) : fe % g.f_nb);
    };
    auto geom_of = [&](int nb, int q, float xn[3], float rn[9]) {
      load_geom_record(nbg_rs, q, xn, rn);
    };
    // Software pipeline (as in the wave-pair kernel): neighbour ids are fetched two chunks ahead and geometry records
    // one chunk ahead, and the chunk's own feature words go out at its top and are only turned into MFMA fragments
    // where the first product needs them -- no load result is needed by the instructions right behind the load (the
    // first version converted the words where they were loaded: one full memory latency per k-step with nothing of
    // this wavefront to overlap it).
    int nb_b = 0, q_a = 0;
    float xn_nx[3], rn_nx[9];
    if (n_total > 0) {
      const int nb_a = nbr_of(0);
      nb_b = nbr_of(32);
      q_a = row_of(nb_a, 0);
      geom_of(nb_a, q_a, xn_nx, rn_nx);
    }
    for (int c0 = 0; c0 < n_total; c0 += 32) {
      const int cnt = min(32, n_total - c0);
      // rows past the end of the edge list are read out of bounds (raw buffer loads return 0), so phi needs no mask
      const int qoff = c0 + kcol < n_total ? q_a * row_bytes : kOobOffset;
      float xn[3], rn[9], d[9];
#pragma unroll
      for (int i = 0; i < 3; ++i) xn[i] = xn_nx[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) rn[i] = rn_nx[i];
      const int q_b = row_of(nb_b, c0 + 32);
      const int nb_q = nb_b;
      nb_b = nbr_of(c0 + 64);

      // gathered feature words of the chunk's two k-steps (shared by the FC rows)
      uint32_t fw[2][VW][8];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int src_off = __builtin_amdgcn_ds_bpermute(hb + 4 * acc_row(8 * s + j, 0), qoff);
          const int voff = ch_ok[0] ? src_off + cb4[0] : kOobOffset;
          if constexpr (VW == 4) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(feat_rs, voff, 0, 0);
            fw[s][0][j] = v[0], fw[s][1][j] = v[1], fw[s][2][j] = v[2], fw[s][3][j] = v[3];
          } else if constexpr (VW == 2) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(feat_rs, voff, 0, 0);
            fw[s][0][j] = v[0], fw[s][1][j] = v[1];
          } else {
            fw[s][0][j] = __builtin_amdgcn_raw_buffer_load_b32(feat_rs, voff, 0, 0);
          }
        }
      }
      geom_of(nb_q, q_b, xn_nx, rn_nx);
      q_a = q_b;

      if (!g.transposed)
        edge_descriptor(xn, rn, yc, rc, rho, d);
      else
        edge_descriptor(yc, rc, xn, rn, rho, d);

      // the chunk as MlpOperand + single_frame write it (the stream1 kernel takes those; here the helpers cost registers)
      u32x4 own_hi, own_lo, oth_hi, oth_lo;
      frags_from_floats(d, own_hi, own_lo);
      {
        float d8 = d[8];
        if constexpr (FC == 2) {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(d8), __float_as_uint(d8), false, false);
          d8 = __uint_as_float(h ? sw[0] : sw[1]);
        }
        uint32_t p_hi, p_lo;
        split2(d8, 1.0f, p_hi, p_lo);
        oth_hi = u32x4{p_hi, 0u, 0u, 0u};
        oth_lo = u32x4{p_lo, 0u, 0u, 0u};
      }
      u32x4 fa_hi[2][VW], fa_lo[2][VW];
#pragma unroll
      for (int a = 0; a < FC; ++a) {
        const bool dims07 = FC == 1 ? h == 0 : h == a;
        u32x4 a_hi, a_lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a_hi[i] = dims07 ? own_hi[i] : oth_hi[i];
          a_lo[i] = dims07 ? own_lo[i] : oth_lo[i];
        }
        const u32x4 wb_hi = *reinterpret_cast<const u32x4*>(&lds_w[a][0][lane][0]);
        const u32x4 wb_lo = *reinterpret_cast<const u32x4*>(&lds_w[a][1][lane][0]);
        f32x16 phi = mfma_bf16x3(a_hi, a_lo, wb_hi, wb_lo, zero16());
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (s * 16 < cnt) {
            u32x4 b_hi, b_lo;
            gelu_frags(phi, s, b_hi, b_lo);
#pragma unroll
            for (int t = 0; t < VW; ++t) {
              if (a == 0) frags_from_words(fw[s][t], fa_hi[s][t], fa_lo[s][t]);
              acc[a][t] = mfma_bf16x3(fa_hi[s][t], fa_lo[s][t], b_hi, b_lo, acc[a][t]);
            }
          }
        }
      }
    }
    // acc[a][t] register r, lane (kcol, h) = T[row a][cbase + VW*acc_row(r,h) + t][kcol].  The values go to the sink in
    // pairs of ADJACENT channels where the layout has them in one lane (what the 3-byte row format stores together):
    // registers r, r + 1 of one tile at one channel per lane (VW = 1), tiles 0 and 1 of one register at two (VW = 2).
#pragma unroll
    for (int a = 0; a < FC; ++a) {
      if constexpr (VW == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ch0 = cbase + 2 * acc_row(r, h);
          sink(a, ch0, ch0 + 1, acc[a][0][r], acc[a][1][r], FULL || ch0 < channels, FULL || ch0 + 1 < channels);
        }
      } else {
#pragma unroll
        for (int t = 0; t < VW; ++t)
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const int ch0 = cbase + VW * acc_row(r, h) + t, ch1 = cbase + VW * acc_row(r + 1, h) + t;
            sink(a, ch0, ch1, acc[a][t][r], acc[a][t][r + 1], FULL || ch0 < channels, FULL || ch1 < channels);
          }
      }
    }
  }
}


}  // namespace se3
