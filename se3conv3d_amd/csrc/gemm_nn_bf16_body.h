// Body of gemm_nn_bf16_kernel<OUT_MODE, FAST, NB> (gemm_bf16.hip); LDS images: as[2][BM][A_LD], bsh / bsl[2][BNW][B_LD].
// Included inside a function whose scope holds the kernel's parameters by their names, the LDS images named below and
// SE3_GRID_BLOCK (the workgroup's index in its grid: blockIdx for the stand-alone kernel, a role's virtual index in the shared
// launch of backward's dense products, bwd_dense_shared_kernel).  A text and not a function on purpose: as an inlined function
// the stand-alone kernels' device code moves (operand order, the waits of the checked tail: profiles/bwd_dense_shared.txt).
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl = lane & 31, h = lane >> 5;
  // (row blocks last-to-first -- A was written front-to-back just before, its tail is still in the memory-side cache --
  // was measured: no difference, 0.245 ms either way)
  const int64_t m0 = (int64_t)SE3_GRID_BLOCK.x * BM;
  const int n0 = SE3_GRID_BLOCK.y * BNW;
  const bool a_vec = (k % 4) == 0;
  const int kt_begin = SE3_GRID_BLOCK.z * kt_per_split;
  const int nk = min(kp / BK - kt_begin, kt_per_split);  // k-tiles of this block (> 0 by construction)

  struct Tile { u32x4 a0, a1, a2, a3, bh[NB], bl[NB]; };
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(a), (short)0, FAST ? (int)(uint32_t)(m * k * 4) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t bh_rs = weight_plane_rsrc(bt_hi, n, kp, FAST), bl_rs = weight_plane_rsrc(bt_lo, n, kp, FAST);
  // Every block walks its k-tiles from a different starting phase (the sum is order-independent up to
  // rounding): with a common phase all resident blocks read the same 128-byte column strip of their
  // 8 KB rows at the same time, which concentrates the traffic on a few HBM channels.
  const int phase = FAST ? (int)((SE3_GRID_BLOCK.x * 5u) % (unsigned)nk) : 0;
  auto load_tile = [&](Tile& t, int kt_seq) {
    int kt = kt_seq + phase;
    if (kt >= nk) kt -= nk;
    const int k0 = (kt_begin + kt) * BK;
    const int row = tid >> 3, kq = (tid & 7) * 4;
    if constexpr (FAST) {
      const uint32_t aoff = (uint32_t)(((m0 + row) * k + k0 + kq) * 4);  // rows >= m fall outside the buffer -> 0
      const uint32_t rstep = (uint32_t)k * 32u * 4u;
      t.a0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, aoff, 0, 0));
      t.a1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, aoff + rstep, 0, 0));
      t.a2 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, aoff + 2 * rstep, 0, 0));
      t.a3 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, aoff + 3 * rstep, 0, 0));
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const uint32_t boff = (uint32_t)((((int64_t)(n0 + 64 * nb + (tid >> 2))) * kp + k0 + (tid & 3) * 8) * 2);
        t.bh[nb] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(bh_rs, boff, 0, 0));
        t.bl[nb] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(bl_rs, boff, 0, 0));
      }
      return;
    }
    const uint32_t* ap = a + (m0 + row) * k + k0 + kq;
    const int64_t avail = k - (k0 + kq);
    t.a0 = ld4_words(ap, m0 + row < m ? avail : 0, a_vec);
    t.a1 = ld4_words(ap + (int64_t)32 * k, m0 + row + 32 < m ? avail : 0, a_vec);
    t.a2 = ld4_words(ap + (int64_t)64 * k, m0 + row + 64 < m ? avail : 0, a_vec);
    t.a3 = ld4_words(ap + (int64_t)96 * k, m0 + row + 96 < m ? avail : 0, a_vec);
    const int kq8 = (tid & 3) * 8;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int nl = 64 * nb + (tid >> 2);
      const bool ok = n0 + nl < n;
      const int64_t boff = (int64_t)(ok ? n0 + nl : 0) * kp + k0 + kq8;
      const u32x4 vh = *reinterpret_cast<const u32x4*>(bt_hi + boff), vl = *reinterpret_cast<const u32x4*>(bt_lo + boff);
      t.bh[nb] = ok ? vh : zero4;
      t.bl[nb] = ok ? vl : zero4;
    }
  };
  f32x16 acc[2 * NB];
#pragma unroll
  for (int c = 0; c < 2 * NB; ++c) acc[c] = zero16();
  auto store_tile = [&](const Tile& t, int buf) {
    const int row = tid >> 3, kq = (tid & 7) * 4;
    *reinterpret_cast<u32x4*>(&as[buf][row][kq]) = t.a0;
    *reinterpret_cast<u32x4*>(&as[buf][row + 32][kq]) = t.a1;
    *reinterpret_cast<u32x4*>(&as[buf][row + 64][kq]) = t.a2;
    *reinterpret_cast<u32x4*>(&as[buf][row + 96][kq]) = t.a3;
    const int kq8 = (tid & 3) * 8;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      *reinterpret_cast<u32x4*>(&bsh[buf][64 * nb + (tid >> 2)][kq8]) = t.bh[nb];
      *reinterpret_cast<u32x4*>(&bsl[buf][64 * nb + (tid >> 2)][kq8]) = t.bl[nb];
    }
  };

  auto compute = [&](int buf) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kk = 16 * s + 8 * h;
      const u32x4 w0 = *reinterpret_cast<const u32x4*>(&as[buf][wave * 32 + rl][kk]);
      const u32x4 w1 = *reinterpret_cast<const u32x4*>(&as[buf][wave * 32 + rl][kk + 4]);
      const u32x4 a_hi = {pair_hi(w0[0], w0[1]), pair_hi(w0[2], w0[3]), pair_hi(w1[0], w1[1]), pair_hi(w1[2], w1[3])};
      const u32x4 a_lo = {pair_lo(w0[0], w0[1]), pair_lo(w0[2], w0[3]), pair_lo(w1[0], w1[1]), pair_lo(w1[2], w1[3])};
      nn_mfma_tiles<NB>(a_hi, a_lo, bsh, bsl, buf, kk, rl, acc);
    }
  };
  // k-tile kt lives in register set (kt mod DEPTH) until it is written to LDS buffer (kt & 1).  The kernel's
  // occupancy is set by its LDS tiles (2 blocks per CU), which leaves 256 VGPRs per wavefront: they hold DEPTH
  // tiles in flight.  Measured on MI355X: 3, 4, 6 and 8 tiles give the same time, and so does the kernel with
  // everything but the A loads removed (a diagnostic build of round 1): 0.245 ms for 1.07 GB = 4.4 TB/s, while the same walk
  // over a buffer that was not just written by the previous kernel reads at 5.8-6.3 TB/s (tools/probes/): the
  // producer's dirty lines are still draining from L2 / the memory-side cache into HBM while this kernel reads.
  constexpr int DEPTH = kGemmDepth;
  static_assert(DEPTH % 2 == 0, "the LDS buffer parity of a step must be a compile-time constant");
  Tile t[DEPTH];
#pragma unroll
  for (int u = 0; u < DEPTH; ++u)
    if (u < nk) load_tile(t[u], u);
  store_tile(t[0], 0);
  __syncthreads();
  // steady state without any condition around the loads (conditional loads make the compiler drain
  // vmcnt(0) every step), then a checked tail
  int kt0 = 0;
  for (; kt0 + 2 * DEPTH <= nk; kt0 += DEPTH) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      load_tile(t[u], kt0 + u + DEPTH);
      compute(u & 1);
      store_tile(t[(u + 1) % DEPTH], (u & 1) ^ 1);
      __syncthreads();
    }
  }
  for (; kt0 < nk; kt0 += DEPTH) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int kt = kt0 + u;
      if (kt < nk) {
        if (kt + DEPTH < nk) load_tile(t[u], kt + DEPTH);
        compute(u & 1);
        if (kt + 1 < nk) store_tile(t[(u + 1) % DEPTH], (u & 1) ^ 1);
        __syncthreads();
      }
    }
  }

  nn_store_acc<OUT_MODE, NB>(acc, c, m, n, m0, n0, wave, rl, h, alpha_num, alpha_scale, SE3_GRID_BLOCK.z);
