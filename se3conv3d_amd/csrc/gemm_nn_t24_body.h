// Body of gemm_nn_t24_kernel<OUT_MODE, NB> (gemm_bf16.hip); LDS: the launch's dynamic LDS, gemm_nn_t24_lds_bytes(NB) of it.
// Included inside a function whose scope holds the kernel's parameters by their names, the LDS images named below and
// SE3_GRID_BLOCK (the workgroup's index in its grid: blockIdx for the stand-alone kernel, a role's virtual index in the shared
// launch of backward's dense products, bwd_dense_shared_kernel).  A text and not a function on purpose: as an inlined function
// the stand-alone kernels' device code moves (operand order, the waits of the checked tail: profiles/bwd_dense_shared.txt).
  constexpr int BNW = BN * NB;
  constexpr int RB = BM;           // rows per workgroup
  constexpr int RP = 32;           // rows one load pass of the hi plane covers (8 threads per row): 4 passes = RB rows
  constexpr int RPL = 64;          // rows one load pass of the lo plane covers (4 threads per row): 2 passes = RB rows
  constexpr int CP = kWeightPassCols, NBP = 2 * NB;
  // one block of LDS, carved into the four tile images
  constexpr int kAsh = 2 * RB * (BK + 8) * 2, kAsl = 2 * RB * (BK + 16), kBs = 2 * BNW * B_LD * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // gemm_nn_t24_lds_bytes: 52 / 72 KB
  auto ash = reinterpret_cast<uint16_t(*)[RB][BK + 8]>(smem);                    // [2][RB][BK + 8], 80-byte pitch
  auto asl = reinterpret_cast<uint8_t(*)[RB][BK + 16]>(smem + kAsh);             // [2][RB][BK + 16], 48-byte pitch
  auto bsh = reinterpret_cast<uint16_t(*)[BNW][B_LD]>(smem + kAsh + kAsl);       // [2][BNW][B_LD]
  auto bsl = reinterpret_cast<uint16_t(*)[BNW][B_LD]>(smem + kAsh + kAsl + kBs);
  // (`& 255` changes no value at 256 threads, but without it the compiler allocates registers differently: kept, so that
  // the kernel stays the code that was measured)
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int rl = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)SE3_GRID_BLOCK.x * RB;
  const int n0 = SE3_GRID_BLOCK.y * BNW;
  const int ns = min(k / 64 - (int)SE3_GRID_BLOCK.z * st_per_split, st_per_split);  // super tiles of this workgroup (> 0 by construction)
  const int st_begin = SE3_GRID_BLOCK.z * st_per_split;

  struct Super { u32x4 ah[4], al[2], bh[NBP], bl[NBP]; };
  const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a), (short)0, (int)(uint32_t)(m * k * 3), 0x00020000);
  const __amdgpu_buffer_rsrc_t bh_rs = weight_plane_rsrc(bt_hi, n, k), bl_rs = weight_plane_rsrc(bt_lo, n, k);
  const int phase = (int)((SE3_GRID_BLOCK.x * 5u) % (unsigned)ns);  // see gemm_nn_bf16_kernel
  const uint32_t rb = (uint32_t)k * 3u;
  const int hsel = (tid >> 2) & 1, lsel = (tid >> 1) & 1;
  auto load_super = [&](Super& t, int seq) {
    int st = seq + phase;
    if (st >= ns) st -= ns;
    const uint32_t k0 = (uint32_t)(st_begin + st) * 64u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint32_t off = (uint32_t)(m0 + p * RP + (tid >> 3)) * rb + k0 * 2u + (uint32_t)((tid & 7) ^ ((p & 1) << 2)) * 16u;
      t.ah[p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, off, 0, 0));
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint32_t off = (uint32_t)(m0 + p * RPL + (tid >> 2)) * rb + (uint32_t)k * 2u + k0 + (uint32_t)((tid & 3) ^ (p << 1)) * 16u;
      t.al[p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, off, 0, 0));
    }
    // (the weight loads stay written out here and in gemm_nn_t16_kernel: as a shared function the offset is associated
    // otherwise -- k0 joins the thread's piece, not the row -- and waits move inside the k loop, profiles/gemm_nn_pieces.txt)
#pragma unroll
    for (int j = 0; j < NBP; ++j) {  // pass j: columns CP * j + (tid >> 3); passes alternate which 32-k half a thread holds
      const uint32_t off = ((uint32_t)(n0 + CP * j + (tid >> 3)) * (uint32_t)k + k0 + (uint32_t)((tid & 7) ^ ((j & 1) << 2)) * 8u) * 2u;
      t.bh[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(bh_rs, off, 0, 0));
      t.bl[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(bl_rs, off, 0, 0));
    }
  };
  // the 32-k half `hf` of a super tile -> LDS buffer `buf`: pieces whose column bit 2 (hi, B) / bit 1 (lo) equals hf
  auto store_half = [&](const Super& t, int hf, int buf) {
    const bool q = (hf ^ hsel) != 0, ql = (hf ^ lsel) != 0;
    const int r8 = tid >> 3, c4 = (tid & 3) * 8;
    *reinterpret_cast<u32x4*>(&ash[buf][(q ? RP : 0) + r8][c4]) = q ? t.ah[1] : t.ah[0];
    *reinterpret_cast<u32x4*>(&ash[buf][(q ? 3 * RP : 2 * RP) + r8][c4]) = q ? t.ah[3] : t.ah[2];
    *reinterpret_cast<u32x4*>(&asl[buf][(ql ? RPL : 0) + (tid >> 2)][(tid & 1) * 16]) = ql ? t.al[1] : t.al[0];
    nn_store_weights_half<NB>(t.bh, t.bl, bsh, bsl, buf, q, r8, c4);
  };
  f32x16 acc[2 * NB];
#pragma unroll
  for (int ct = 0; ct < 2 * NB; ++ct) acc[ct] = zero16();
  auto compute = [&](int buf) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kk = 16 * s + 8 * h;
      // the hi fragment is one 16-byte read; the lo fragment is rebuilt from the 8 lo bytes (7 VALU per pair)
      const u32x4 a_hi = *reinterpret_cast<const u32x4*>(&ash[buf][wave * 32 + rl][kk]);
      const uint32_t* lp = reinterpret_cast<const uint32_t*>(&asl[buf][wave * 32 + rl][kk]);
      const uint32_t l0 = lp[0], l1 = lp[1];
      const u32x4 a_lo = {t24_lo_word<0>(a_hi[0], l0), t24_lo_word<2>(a_hi[1], l0), t24_lo_word<0>(a_hi[2], l1),
                          t24_lo_word<2>(a_hi[3], l1)};
      nn_mfma_tiles<NB>(a_hi, a_lo, bsh, bsl, buf, kk, rl, acc);
    }
  };
  // Two super tiles in registers (= the 4 k-tiles in flight of the kernel above).  Step A computes the first half
  // while the second goes to LDS buffer 1; step B computes the second half, stores the next super tile's first half
  // to buffer 0 and refills the register set that just emptied.
  Super t0, t1;
  load_super(t0, 0);
  if (ns > 1) load_super(t1, 1);
  store_half(t0, 0, 0);
  __syncthreads();
#define SE3_T24_STEP(CUR, NEXT, ST)                       \
  compute(0);                                             \
  store_half(CUR, 1, 1);                                  \
  __syncthreads();                                        \
  if ((ST) + 2 < ns) load_super(CUR, (ST) + 2);           \
  compute(1);                                             \
  if ((ST) + 1 < ns) store_half(NEXT, 0, 0);              \
  __syncthreads();
#define SE3_T24_STEP_FULL(CUR, NEXT, ST) \
  compute(0);                            \
  store_half(CUR, 1, 1);                 \
  __syncthreads();                       \
  load_super(CUR, (ST) + 2);             \
  compute(1);                            \
  store_half(NEXT, 0, 0);                \
  __syncthreads();
  int st = 0;
  const int prio_slot = wave_slot_id();
  for (; st + 4 <= ns; st += 2) {  // no conditions around the loads (see gemm_nn_bf16_kernel)
    rotate_priority(prio_slot + (st >> 1));
    SE3_T24_STEP_FULL(t0, t1, st)
    SE3_T24_STEP_FULL(t1, t0, st + 1)
  }
  for (; st < ns; st += 2) {
    SE3_T24_STEP(t0, t1, st)
    if (st + 1 < ns) {
      SE3_T24_STEP(t1, t0, st + 1)
    }
  }
#undef SE3_T24_STEP
#undef SE3_T24_STEP_FULL

  nn_store_acc<OUT_MODE, NB>(acc, c, m, n, m0, n0, wave, rl, h, alpha_num, alpha_scale, SE3_GRID_BLOCK.z);
