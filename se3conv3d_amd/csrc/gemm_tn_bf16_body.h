// Body of gemm_tn_bf16_kernel<FAST, AFMT> (gemm_bf16.hip); LDS images: at, ath, atl, bt, bth, btl (see the kernel).
// Included inside a function whose scope holds the kernel's parameters by their names, the LDS images named below and
// SE3_GRID_BLOCK (the workgroup's index in its grid: blockIdx for the stand-alone kernel, a role's virtual index in the shared
// launch of backward's dense products, bwd_dense_shared_kernel).  A text and not a function on purpose: as an inlined function
// the stand-alone kernels' device code moves (operand order, the waits of the checked tail: profiles/bwd_dense_shared.txt).
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl = lane & 31, h = lane >> 5;
  const int ka0 = SE3_GRID_BLOCK.x * 128;
  const int n0 = SE3_GRID_BLOCK.y * BN;
  const int64_t mb = (int64_t)SE3_GRID_BLOCK.z * chunk;
  const int64_t me = min(m, mb + chunk);
  const bool b_vec = (n % 4) == 0;
  const int64_t nst = me > mb ? (me - mb + BK - 1) / BK : 0;

  struct Stage { u32x4 a0, a1, a2, a3, b0, b1; };
  const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(a), (short)0, FAST ? (int)(uint32_t)(me * gemm_a_row_bytes(AFMT, ka)) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t b_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(b), (short)0, FAST ? (int)(uint32_t)(me * n * 4) : 0, 0x00020000);
  const int arow = tid >> 5, acq = (tid & 31) * 4, brow = tid >> 4, bcq = (tid & 15) * 4;
  const bool a_ok = ka0 + acq < ka, b_ok = n0 + bcq < n;
  auto load_stage = [&](Stage& t, int64_t st) {
    const int64_t mm = mb + st * BK;
    if constexpr (A16) {
      const uint32_t oob = 0xfffffff0u;
      const uint32_t rb = (uint32_t)gemm_a_row_bytes(AFMT, ka);
      constexpr int kNtLoad = 2;
      // mantissas: 32 rows x 256 B = 2 pieces of 16 B per thread (rows tid >> 4 and + 16, piece tid & 15 = 8 mantissas =
      // blocks 2 pc, 2 pc + 1 of the 128 columns); their exponent bytes are adjacent in the plane (t16_exp_pos: bit 0)
      const bool h_ok = ka0 + (tid & 15) * 8 < ka;
      const uint32_t ho = (uint32_t)(mm + (tid >> 4)) * rb + (uint32_t)(ka0 + (tid & 15) * 8) * 2u;
      const uint32_t eo = (uint32_t)(mm + (tid >> 4)) * rb + (uint32_t)ka * 2u + (uint32_t)t16_exp_pos((ka0 + (tid & 15) * 8) >> 2);
      const uint32_t bo = b_ok ? (uint32_t)(((mm + brow) * n + n0 + bcq) * 4) : oob;
      const uint32_t bs16 = (uint32_t)n * 64u;
      t.a0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, h_ok ? ho : oob, 0, kNtLoad));
      t.a1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, h_ok ? ho + 16u * rb : oob, 0, kNtLoad));
      t.a2[0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(a_rs, h_ok ? eo : oob, 0, kNtLoad);
      t.a2[1] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(a_rs, h_ok ? eo + 16u * rb : oob, 0, kNtLoad);
      t.b0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rs, bo, 0, 0));
      t.b1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rs, b_ok ? bo + bs16 : oob, 0, 0));
    } else if constexpr (A24) {
      const uint32_t oob = 0xfffffff0u;
      const uint32_t rb = (uint32_t)ka * 3u;
      // hi: 32 rows x 256 B = 2 pieces of 16 B per thread; lo: 32 rows x 128 B = 1 piece per thread.  The rows are
      // read once: non-temporal loads keep them from displacing the g tiles the 16 column blocks share in L2
      // (0.178 -> 0.170 ms; the same hint on the NN GEMM's A stream costs it 0.01 ms)
      constexpr int kNtLoad = 2;
      const bool h_ok = ka0 + (tid & 15) * 8 < ka, l_ok = ka0 + (tid & 7) * 16 < ka;
      const uint32_t ho = (uint32_t)(mm + (tid >> 4)) * rb + (uint32_t)(ka0 + (tid & 15) * 8) * 2u;
      const uint32_t lo = (uint32_t)(mm + (tid >> 3)) * rb + (uint32_t)ka * 2u + (uint32_t)(ka0 + (tid & 7) * 16);
      const uint32_t bo = b_ok ? (uint32_t)(((mm + brow) * n + n0 + bcq) * 4) : oob;
      const uint32_t bs16 = (uint32_t)n * 64u;
      t.a0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, h_ok ? ho : oob, 0, kNtLoad));
      t.a1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, h_ok ? ho + 16u * rb : oob, 0, kNtLoad));
      t.a2 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, l_ok ? lo : oob, 0, kNtLoad));
      t.b0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rs, bo, 0, 0));
      t.b1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rs, b_ok ? bo + bs16 : oob, 0, 0));
    } else if constexpr (FAST) {
      const uint32_t oob = 0xfffffff0u;  // beyond num_records: the load returns 0
      const uint32_t ao = a_ok ? (uint32_t)(((mm + arow) * ka + ka0 + acq) * 4) : oob;
      const uint32_t bo = b_ok ? (uint32_t)(((mm + brow) * n + n0 + bcq) * 4) : oob;
      const uint32_t as8 = (uint32_t)ka * 32u, bs16 = (uint32_t)n * 64u;
      t.a0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, ao, 0, 0));
      t.a1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, a_ok ? ao + as8 : oob, 0, 0));
      t.a2 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, a_ok ? ao + 2 * as8 : oob, 0, 0));
      t.a3 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, a_ok ? ao + 3 * as8 : oob, 0, 0));
      t.b0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rs, bo, 0, 0));
      t.b1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rs, b_ok ? bo + bs16 : oob, 0, 0));
    } else {
      u32x4* ta[4] = {&t.a0, &t.a1, &t.a2, &t.a3};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int64_t gr = mm + p * 8 + arow;
        *ta[p] = ld4_words(a + gr * ka + ka0 + acq, gr < me ? ka - (ka0 + acq) : 0, true);
      }
      u32x4* tb[2] = {&t.b0, &t.b1};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int64_t gr = mm + p * 16 + brow;
        *tb[p] = ld4_words(b + gr * n + n0 + bcq, gr < me ? n - (n0 + bcq) : 0, b_vec);
      }
    }
  };
  // the hi / lo halves of a stage's B words (rows brow and brow + 16) into the 16-bit images of the row-plane forms (A16, A24)
  auto store_b_planes = [&](const Stage& t, int buf) {
    *reinterpret_cast<u32x2*>(&bth[buf][brow][bcq]) = u32x2{pair_hi(t.b0[0], t.b0[1]), pair_hi(t.b0[2], t.b0[3])};
    *reinterpret_cast<u32x2*>(&btl[buf][brow][bcq]) = u32x2{pair_lo(t.b0[0], t.b0[1]), pair_lo(t.b0[2], t.b0[3])};
    *reinterpret_cast<u32x2*>(&bth[buf][brow + 16][bcq]) = u32x2{pair_hi(t.b1[0], t.b1[1]), pair_hi(t.b1[2], t.b1[3])};
    *reinterpret_cast<u32x2*>(&btl[buf][brow + 16][bcq]) = u32x2{pair_lo(t.b1[0], t.b1[1]), pair_lo(t.b1[2], t.b1[3])};
  };
  auto store_stage = [&](const Stage& t, int buf) {
    if constexpr (A16) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const u32x4 mw = p ? t.a1 : t.a0;
        const uint32_t e2 = t.a2[p];
        u32x4 vh, vl;
        t16_unpack8(mw, e2, vh, vl);
        *reinterpret_cast<u32x4*>(&ath[buf][16 * p + (tid >> 4)][(tid & 15) * 8]) = vh;
        *reinterpret_cast<u32x4*>(&atl[buf][16 * p + (tid >> 4)][(tid & 15) * 8]) = vl;
      }
      store_b_planes(t, buf);
    } else if constexpr (A24) {
      *reinterpret_cast<u32x4*>(&ath[buf][tid >> 4][(tid & 15) * 8]) = t.a0;
      *reinterpret_cast<u32x4*>(&ath[buf][16 + (tid >> 4)][(tid & 15) * 8]) = t.a1;
      u32x4 e0, e1;  // 16 lo bytes -> 16 half-words
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        e0[2 * i] = __builtin_amdgcn_perm(0u, t.a2[i], 0x0c010c00u), e0[2 * i + 1] = __builtin_amdgcn_perm(0u, t.a2[i], 0x0c030c02u);
        e1[2 * i] = __builtin_amdgcn_perm(0u, t.a2[2 + i], 0x0c010c00u), e1[2 * i + 1] = __builtin_amdgcn_perm(0u, t.a2[2 + i], 0x0c030c02u);
      }
      *reinterpret_cast<u32x4*>(&atl[buf][tid >> 3][(tid & 7) * 16]) = e0;
      *reinterpret_cast<u32x4*>(&atl[buf][tid >> 3][(tid & 7) * 16 + 8]) = e1;
      store_b_planes(t, buf);
    } else {
      *reinterpret_cast<u32x4*>(&at[buf][arow][acq]) = t.a0;
      *reinterpret_cast<u32x4*>(&at[buf][arow + 8][acq]) = t.a1;
      *reinterpret_cast<u32x4*>(&at[buf][arow + 16][acq]) = t.a2;
      *reinterpret_cast<u32x4*>(&at[buf][arow + 24][acq]) = t.a3;
      *reinterpret_cast<u32x4*>(&bt[buf][brow][bcq]) = t.b0;
      *reinterpret_cast<u32x4*>(&bt[buf][brow + 16][bcq]) = t.b1;
    }
  };

  f32x16 acc0 = zero16(), acc1 = zero16();
  auto compute = [&](int buf) {
    if constexpr (A24) {
      const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = (lane & 3) * 4;
      const int col = 16 * (grp & 1) + p4;  // this lane's address: row q of the block, 4 columns from here
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int r0 = 16 * s + 8 * (grp >> 1) + q;
        const u32x4 a_hi = lds_frag_tr16(&ath[buf][r0][wave * 32 + col], &ath[buf][r0 + 4][wave * 32 + col]);
        const u32x4 lw = lds_frag_tr16(&atl[buf][r0][wave * 32 + col], &atl[buf][r0 + 4][wave * 32 + col]);
        u32x4 a_lo = lw;  // T16: the lo plane holds the bf16 lo operand itself
        if constexpr (!A16)
          a_lo = u32x4{t24_lo_word<0, 2>(a_hi[0], lw[0]), t24_lo_word<0, 2>(a_hi[1], lw[1]),
                       t24_lo_word<0, 2>(a_hi[2], lw[2]), t24_lo_word<0, 2>(a_hi[3], lw[3])};
        u32x4 b_hi = lds_frag_tr16(&bth[buf][r0][col], &bth[buf][r0 + 4][col]);
        u32x4 b_lo = lds_frag_tr16(&btl[buf][r0][col], &btl[buf][r0 + 4][col]);
        acc0 = mfma_bf16x3(a_hi, a_lo, b_hi, b_lo, acc0);
        b_hi = lds_frag_tr16(&bth[buf][r0][32 + col], &bth[buf][r0 + 4][32 + col]);
        b_lo = lds_frag_tr16(&btl[buf][r0][32 + col], &btl[buf][r0 + 4][32 + col]);
        acc1 = mfma_bf16x3(a_hi, a_lo, b_hi, b_lo, acc1);
      }
      return;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint32_t wa[8], wb0[8], wb1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = 16 * s + 8 * h + j;
        wa[j] = at[buf][row][wave * 32 + rl];
        wb0[j] = bt[buf][row][rl];
        wb1[j] = bt[buf][row][32 + rl];
      }
      u32x4 a_hi, a_lo, b_hi, b_lo;
      frags_from_words(wa, a_hi, a_lo);
      frags_from_words(wb0, b_hi, b_lo);
      acc0 = mfma_bf16x3(a_hi, a_lo, b_hi, b_lo, acc0);
      frags_from_words(wb1, b_hi, b_lo);
      acc1 = mfma_bf16x3(a_hi, a_lo, b_hi, b_lo, acc1);
    }
  };
  if (nst > 0) {
    Stage t0, t1, t2;
    load_stage(t0, 0);
    if (1 < nst) load_stage(t1, 1);
    if (2 < nst) load_stage(t2, 2);
    store_stage(t0, 0);
    __syncthreads();
#define SE3_TN_STEP_FULL(ST, CUR, NEXT) \
  load_stage(CUR, (ST) + 3);            \
  compute((int)((ST) & 1));             \
  store_stage(NEXT, (int)((ST) & 1) ^ 1); \
  __syncthreads();
#define SE3_TN_STEP(ST, CUR, NEXT)                                   \
  if ((ST) < nst) {                                                  \
    if ((ST) + 3 < nst) load_stage(CUR, (ST) + 3);                   \
    compute((int)((ST) & 1));                                        \
    if ((ST) + 1 < nst) store_stage(NEXT, (int)((ST) & 1) ^ 1);      \
    __syncthreads();                                                 \
  }
    int64_t st = 0;
    const int prio_slot = wave_slot_id();
    for (; st + 6 <= nst; st += 3) {
      rotate_priority(prio_slot + (int)(st / 3));  // every workgroup of this product is resident for the whole launch (common.h)
      SE3_TN_STEP_FULL(st, t0, t1)
      SE3_TN_STEP_FULL(st + 1, t1, t2)
      SE3_TN_STEP_FULL(st + 2, t2, t0)
    }
    for (; st < nst; st += 3) {
      SE3_TN_STEP(st, t0, t1)
      SE3_TN_STEP(st + 1, t1, t2)
      SE3_TN_STEP(st + 2, t2, t0)
    }
#undef SE3_TN_STEP
#undef SE3_TN_STEP_FULL
  }
  float* out = partials + (int64_t)SE3_GRID_BLOCK.z * ka * n;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kq = ka0 + wave * 32 + acc_row(r, h);
    if (kq < ka) {
      const int row = A16 ? t16_k_of(kq) : (A24 ? t24_k_of(kq) : kq);
      if (n0 + rl < n) out[(int64_t)row * n + n0 + rl] = acc0[r];
      if (n0 + 32 + rl < n) out[(int64_t)row * n + n0 + 32 + rl] = acc1[r];
    }
  }
