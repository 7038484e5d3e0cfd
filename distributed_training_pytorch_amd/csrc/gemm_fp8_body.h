// The body of the pipelined FP8 GEMM kernels of gemm_fp8.hip up to the epilogue passes: included inside
// gemm_fp8_kernel and gemm_fp8_qout_kernel, which differ only in the passes that follow (text inclusion,
// not a shared function: the instances without a quantised output compile to the code they had before
// the quantising ones existed).  Expects FA, X32, SPLIT and the kernel argument `a`; leaves lds, e, acc,
// ebuf, bias, m0, wr, ncol, vec, lane, wave and tid for the passes.
  __shared__ __align__(16) char lds[kLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;

  DtpGemmArgs e{};  // the epilogue's view of the problem (gemm_epi.h)
  e.M = a.M;
  e.N = a.N;
  e.K = a.K;
  e.dtype = DTP_DT_BF16;
  if constexpr (SPLIT) {  // raw partial sums: no bias, aux, act or accumulate, alpha = 1
    e.ldc = a.N;
    e.out_dtype = DTP_DT_F32;
    e.splitk = a.splitk;  // (for decode_tile; 1 again before the stores)
    e.alpha = 1.f;
  } else {
    e.C = a.C;
    e.bias = a.bias;
    e.aux = a.aux;
    e.ldc = a.ldc;
    e.ldaux = a.ldaux;
    e.out_dtype = a.out_dtype;
    e.act = a.act;
    e.accumulate = a.accumulate;
    e.splitk = 1;
    e.slope = a.slope;
    e.alpha = *a.sa_inv * *a.sb_inv;
  }

  const TileId id = decode_tile<256, 256>(e);
  const int m0 = id.m0, n0 = id.n0;
  const int ktail = a.K & 127;  // valid bytes of the last K-tile (0: all 128)
  // this block's K-tiles: nk of them from tile kt0 on; the global last K-tile, the only ragged one,
  // is its tile ktl (>= nk: in another slice)
  int nk = (a.K + 127) >> 7, kt0 = 0;
  int ktl = nk - 1;
  if constexpr (SPLIT) {
    const F8Slice sl = f8_slice(nk, a.splitk, id.ks);
    nk = sl.nkt;
    kt0 = sl.t0;
    ktl -= sl.t0;
    e.C = static_cast<float*>(a.work) + static_cast<long long>(id.ks) * a.M * a.N;
    e.splitk = 1;
  }

  uint32_t oSA[2][2], oSB[2][2];
  part_sources(oSA, a.lda, m0, a.M, wave, lane);
  part_sources(oSB, a.ldb, n0, a.N, wave, lane);
  const char* gA = static_cast<const char*>(a.A) + m0 * a.lda + static_cast<uint32_t>(kt0) * 128u;
  const char* gB = static_cast<const char*>(a.B) + n0 * a.ldb + static_cast<uint32_t>(kt0) * 128u;
  // the source chunk of this lane in every DMA instruction (fswz reads row bits 0, 1, 3 =
  // lane bits 3, 4 and wave bit 0: the same for both instructions and both parts)
  const int csrc = (lane & 7) ^ fswz((wave * 8 + (lane >> 3)) & 15);
  const bool dead = ktail && csrc * 16 >= ktail;
  const char* zero = reinterpret_cast<const char*>(&g_zero_chunk);

  // one part (P: 0 = A0, 1 = A1, 2 = B0, 3 = B1) of K-tile `tile` (counted from the block's
  // first) into its buffer, or into the sink past the last tile (same wait accounting every phase)
  auto stage = [&](auto P, int tile) {
    constexpr int p = decltype(P)::value;
    const bool real = tile < nk;
    char* dst = lds + (real ? (tile & 1) * kBuf + p * kPart : kSink) + wave * 1024;
    // 32-bit tile offset (dtp_gemm_fp8 requires each operand < 2 GiB)
    const char* g = (p < 2 ? gA : gB) + static_cast<uint32_t>(real ? tile : 0) * 128u;
    const uint32_t* o = p < 2 ? oSA[p & 1] : oSB[p & 1];
    // the ragged K-tile (a sink slot re-reads tile 0): chunks past K come from the zero block
    // (the unsplit instances keep their own form of the same test: ktl = nk - 1 there)
    const bool cut = dead && (SPLIT ? (real ? tile : 0) == ktl : (real ? tile == nk - 1 : nk == 1));
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(cut ? zero : g + o[i]), (lds_void_t*)(dst + i * 8192), 16, 0, 0);
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;

  // byte offsets of this lane's two fragment chunks (lg and 4 + lg) inside a part;
  // fragment f (16 rows) adds 2048 f
  const int lr = lane & 15, lg = lane >> 4;
  int oA[2], oB[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    oA[h] = ((wr * 64 + lr) * 8 + ((4 * h + lg) ^ fswz(lr))) * 16;
    oB[h] = ((wc * 32 + lr) * 8 + ((4 * h + lg) ^ fswz(lr))) * 16;
  }

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  i32x8 fa[4], fb0[2], fb1[2];
  auto rdA = [&](const char* part) {
#pragma unroll
    for (int f = 0; f < 4; ++f) fa[f] = frag(part, oA, f);
  };
  auto rdB = [&](const char* part, i32x8 (&fb)[2]) {
#pragma unroll
    for (int g = 0; g < 2; ++g) fb[g] = frag(part, oB, g);
  };
  // end of a phase's load segment: retire the part the next phase reads, meet the
  // partner group, then the quadrant's MFMAs at raised priority
  auto mid = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
  };
  auto end = [&]() {
    __builtin_amdgcn_s_setprio(0);
    barrier();
  };
  auto mma = [&](auto QM, auto QN, const i32x8 (&fb)[2]) {
    constexpr int qm = decltype(QM)::value, qn = decltype(QN)::value;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int g = 0; g < 2; ++g)
        acc[4 * qm + f][2 * qn + g] = mma_frag<FA, X32>(fa[f], fb[g], acc[4 * qm + f][2 * qn + g]);
  };
  using Q0 = std::integral_constant<int, 0>;
  using Q1 = std::integral_constant<int, 1>;

  // prologue: B0, A0, B1, A1 of tile 0 and B0 of tile 1 (the order the loop's phases
  // -5 .. -1 would have staged them); vmcnt(6) retires B0 and A0 of tile 0
  stage(P2{}, 0);
  stage(P0{}, 0);
  stage(P3{}, 0);
  stage(P1{}, 0);
  stage(P2{}, 1);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  barrier();
  if (wave >= 4) barrier();  // stagger: waves 4-7 one barrier behind

  for (int u = 0; u < nk; ++u) {
    const char* buf = lds + (u & 1) * kBuf;
    // phase 0: quadrant (0,0)
    rdB(buf + 2 * kPart, fb0);
    rdA(buf);
    stage(P0{}, u + 1);
    mid();
    mma(Q0{}, Q0{}, fb0);
    end();
    // phase 1: quadrant (0,1)
    rdB(buf + 3 * kPart, fb1);
    stage(P3{}, u + 1);
    mid();
    mma(Q0{}, Q1{}, fb1);
    end();
    // phase 2: quadrant (1,1)
    rdA(buf + kPart);
    stage(P1{}, u + 1);
    mid();
    mma(Q1{}, Q1{}, fb1);
    end();
    // phase 3: quadrant (1,0), fragments already in registers
    stage(P2{}, u + 2);
    mid();
    mma(Q1{}, Q0{}, fb0);
    end();
  }
  if (wave < 4) barrier();  // end of the stagger: equal barrier counts
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  barrier();

  // epilogue: LDS-staged 16-byte rows, one pass per row quadrant; the lane's 8 staged
  // columns 8 (lane & 7) .. +8 sit in column quadrant (lane & 7) >> 2
  float* ebuf = reinterpret_cast<float*>(lds) + wave * kEpiWaveFloats;
  const int c8 = lane & 7;
  const int ncol = n0 + (c8 >> 2) * 128 + wc * 32 + 8 * (c8 & 3);
  const uintptr_t cp = reinterpret_cast<uintptr_t>(e.C), ap = reinterpret_cast<uintptr_t>(e.aux);
  const bool vec = ncol + 8 <= e.N && e.ldc % 8 == 0 && (cp & 15) == 0 && (!e.aux || (e.ldaux % 8 == 0 && (ap & 15) == 0));
  float bias[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) bias[c] = (e.bias && ncol + c < e.N) ? e.bias[ncol + c] : 0.f;
