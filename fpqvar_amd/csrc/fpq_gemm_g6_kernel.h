// fpq_gemm_g6_kernel.h - the text of the per-group(128) GEMM kernel with a 6-bit side: the "A6W4" kernels (6-bit activation codes
// against E2M1 weight nibbles) and the "W6" kernels (a 6-bit weight against an E2M1, E1M2 or E3M0 activation) are this one text.
// NOT a header of its own: fpq_gemm_g6.h includes it once per kernel it defines, with
//   FPQ_G6_KERNEL   the kernel's name
//   FPQ_G6_FC1      0: the plain epilogue (+ gate / residual tail); 1 / 2: the fc1 tail (FPQ_GEMM_FC1_TAIL, fpq_gemm_fp4.h; 2: its
//                   NaN-excluding form, FPQ_GEMM_FC1_TAIL_X) - the kernel takes a GemmFc1 behind the GemmEpi and stages the dual
//                   quantizer's bucket table behind the scale tiles
//   FPQ_G6_OUT      (FPQ_G6_FC1 == 0 only) 0: one [T, O] tensor; 1: the SPLIT OUTPUT of GemmEpi's sp_* fields (mat_qkv: q to its own
//                   tensor, k and v into the KV cache's slots), the plain epilogue's values bit for bit, no gate / residual tail;
//                   2: the split output with the Q / K L2 NORM in front of it (FPQ_QK_NORM_ROW, fpq_gemm_fp4.h) - the kernel takes a
//                   GemmQkNorm behind the GemmEpi, its fp32 bias replaces the fp16 one;
//                   3: NO output - the SQUARED-ERROR TAIL (FPQ_GEMM_SQERR_EPILOGUE, fpq_gemm_fp4.h): the plain epilogue's values
//                   against a reference, one fp32 partial per tile - the kernel takes a GemmSqErr behind the GemmEpi (row-major only)
//   FPQ_G6_KM       0: row-major codes and scales (fp16 activation scales); 1: K-MAJOR IMAGES (include/fpq.h) - per side the 4-bit
//                   image [G][rows][64] or the 6-bit image [G][rows][96], the weight's rows dealt and padded to epi.km_w_rows (outs
//                   rounded up to 64), and sa / sw the fp32 scale images [G][T rounded up to 4] / [G][km_w_rows]: every piece of a
//                   stage is 1 KiB contiguous, and the scale tiles come in by LDS-DMA too.  Tsw = float only.
//   FPQ_G6_W4       1: the weight format is fixed to E2M1 (FW = 4) and the template takes <Tsw, MT, NT, FA> - the A6W4 kernels'
//                   signature, so their symbols are what they were; 0: <Tsw, MT, NT, FA, FW>, FW = 2 / 3
// An absent parameter is 0, and the text #undefs all five at its end: an instantiation is the name, the non-zero parameters and
// the #include.
// Either side's tile of a stage and fragment of a lane (32 consecutive k of k-block lane >> 4) come in one of two forms, chosen
// at compile time per side (A4, W4):
//   * nibbles (FA = 4 / FW = 4): gemm_fp4_glds_kernel's 16-row, 1 KiB blocks - glds_chunk_perm, one ds_read_b128 per fragment;
//   * 6-bit codes (2 / 3), activation side: the FP6 kernel's 32-row, 3 KiB super-blocks (fpq_gemm_fp6_kernel.h) - fp6_rot, three
//     ds_read_b64 per fragment; first used against nibbles by the A6W4 kernel;
//   * 6-bit codes, weight side: the FP6 kernel's weight super-blocks, rows dealt over a wavefront's NT tiles; first used by the W6
//     kernel.  (A nibble weight block is dealt the same way.)
// The tile walk, the k-major scale tiles, the lane's bias loads, the software pipeline over a K group and the register epilogues do
// not depend on the forms and are not written here: they are the stages this text shares with gemm_fp4_glds_kernel and
// gemm_fp4_ring_kernel (fpq_gemm_fp4.h, "THE STAGES OF THE PER-GROUP(128) LDS-DMA KERNELS").  What is this text's own: the lane
// offsets and the issue of a stage in the two forms, the fragment readers, and the choice of tail.  Every kernel's machine code
// is, instruction for instruction, what the two families' separate texts gave (profiles/g6_merge_isa.txt) and what this text gave
// with its own copy of the shared stages (profiles/gemm_shared_stages_isa.txt).
#ifndef FPQ_G6_FC1
#define FPQ_G6_FC1 0
#endif
#ifndef FPQ_G6_OUT
#define FPQ_G6_OUT 0
#endif
#ifndef FPQ_G6_KM
#define FPQ_G6_KM 0
#endif
#ifndef FPQ_G6_W4
#define FPQ_G6_W4 0
#endif
#if FPQ_G6_KM
#define FPQ_G6_TSA float
#else
#define FPQ_G6_TSA _Float16
#endif
#if FPQ_G6_W4
template <typename Tsw, int MT, int NT, int FA>
#else
template <typename Tsw, int MT, int NT, int FA, int FW>
#endif
__global__ __launch_bounds__(256, 2) FPQ_NOPK void FPQ_G6_KERNEL(const uint8_t* __restrict__ A, const FPQ_G6_TSA* __restrict__ sa,
                                                                 const uint8_t* __restrict__ W, const Tsw* __restrict__ sw,
                                                                 const _Float16* __restrict__ bias, _Float16* out, int T, int O, int C,
                                                                 GemmEpi epi
#if FPQ_G6_FC1
                                                                 , GemmFc1 xe
#elif FPQ_G6_OUT == 2
                                                                 , GemmQkNorm xe
#elif FPQ_G6_OUT == 3
                                                                 , GemmSqErr xe
#endif
                                                                 ) {
#if FPQ_G6_W4
  constexpr int FW = 4;
#endif
  static_assert(FA == 4 || FA == 2 || FA == 3, "activation format: 4 = FP4 E2M1, 2 = FP6 E2M3 (E1M2 levels), 3 = BF6 E3M2 (E3M0 levels)");
  static_assert(FW == 4 || FW == 2 || FW == 3, "weight format: 4 = FP4 E2M1, 2 = FP6 E2M3 (E1M2 levels), 3 = BF6 E3M2 (E3M0 levels)");
  static_assert(FA != 4 || FW != 4, "one side is 6-bit: the E2M1 x E2M1 product is gemm_fp4_glds_kernel's");
  static_assert(NT == 4, "the epilogue packs a lane's NT results of one row into one 8-byte store");
  constexpr bool A4 = FA == 4, W4 = FW == 4;
  constexpr int WR = 2, WC = 2, BM = 16 * MT * WR, BN = 16 * NT * WC, NTHR = 256;
  static_assert(BM % 64 == 0 && BN % 32 == 0, "whole super-blocks; load_scale_tiles wants the A / W boundary wavefront-uniform");
  constexpr int A_SEG = A4 ? 64 : 96, W_SEG = W4 ? 64 : 96, A_TILE = 16 * A_SEG, W_TILE = 16 * W_SEG;   // bytes of a row per group, of a 16-row tile
  constexpr int APC = BM * A_SEG / 1024, WPC = BN * W_SEG / 1024, NPC = APC + WPC;                     // pieces of A, of W, of a stage
  constexpr int ABYTES = APC * 1024, STAGE = NPC * 1024;
  constexpr int PIECES = (NPC + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int G = C >> 7, a_row_bytes = A4 ? C >> 1 : (C >> 2) * 3, w_row_bytes = W4 ? C >> 1 : (C >> 2) * 3;
  float* lsa = (float*)(smem + 2 * STAGE);   // [G][BM]
  const int Gp = (G + 3) & ~3;
  float* lsw = lsa + Gp * BM;                // [G][BN]
  FPQ_GEMM_TILE_WALK(BM, BN);

  // LDS-DMA sources: a uniform base per operand + a 32-bit lane offset that never changes (see gemm_fp4_glds_kernel); rows past
  // the end of a tensor are clamped to its last row - their products land where the epilogue never stores
#if FPQ_G6_KM
  static_assert(__is_same(Tsw, float), "the k-major scale images are fp32");
  // plane g of an image holds every row's 64 / 96 bytes of group g, chunks in the LDS image's order (no glds_chunk_perm, no fp6_rot
  // here), weight rows in dealt order and padded to km_w_rows: the lane fetches the physical chunk of its image row
  // (gemm_fp4_glds_kernel, fpq_gemm_fp6_kernel.h)
  const int64_t a_step = (int64_t)T * A_SEG, w_step = (int64_t)epi.km_w_rows * W_SEG;
  (void)a_row_bytes, (void)w_row_bytes;
  const uint8_t* const a_base_g = A + (int64_t)t0 * A_SEG;
  const uint8_t* const w_base_g = W + (int64_t)o0 * W_SEG;
  uint32_t voff[PIECES];
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int piece = wave + 4 * i;
    if (piece < APC) {
      if constexpr (A4) {                               // a 16-row block of the 4-bit image
        const int t = t0 + piece * 16 + (lane >> 2);
        voff[i] = (uint32_t)((t < T ? t : T - 1) - t0) * 64u + (uint32_t)((lane & 3) * 16);
      } else {                                          // super-block piece / 3, part piece % 3 of the 6-bit image
        const int sb = piece / 3, ci = (piece % 3) * 64 + lane;
        const int r = ci / 6, pc = ci - 6 * r;          // row inside the super-block, physical chunk
        const int t = t0 + sb * 32 + r;
        voff[i] = (uint32_t)((t < T ? t : T - 1) - t0) * 96u + (uint32_t)(pc * 16);
      }
    } else if constexpr (W4) {                          // the weight side, image row o: the dealing is in the image
      const int o = o0 + (piece - APC) * 16 + (lane >> 2);
      voff[i] = (uint32_t)((o < epi.km_w_rows ? o : epi.km_w_rows - 1) - o0) * 64u + (uint32_t)((lane & 3) * 16);
    } else {
      const int wp = piece - APC, sb = wp / 3, ci = (wp % 3) * 64 + lane;
      const int r = ci / 6, pc = ci - 6 * r;
      const int o = o0 + sb * 32 + r;
      voff[i] = (uint32_t)((o < epi.km_w_rows ? o : epi.km_w_rows - 1) - o0) * 96u + (uint32_t)(pc * 16);
    }
  }
#else
  constexpr int a_step = A_SEG, w_step = W_SEG;   // row-major: a group is the next A_SEG / W_SEG bytes of every row
  const uint8_t* const a_base_g = A + (int64_t)t0 * a_row_bytes;
  const uint8_t* const w_base_g = W + (int64_t)o0 * w_row_bytes;
  uint32_t voff[PIECES];
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int piece = wave + 4 * i;
    if (piece < APC) {
      if constexpr (A4) {                               // a 16-row block of nibbles, natural row order (gemm_fp4_glds_kernel)
        const int q = lane >> 2, kb = (lane & 3) ^ glds_chunk_perm(q);
        const int t = t0 + piece * 16 + q;
        voff[i] = (uint32_t)((t < T ? t : T - 1) - t0) * (uint32_t)a_row_bytes + (uint32_t)(kb * 16);
      } else {                                          // super-block piece / 3, part piece % 3 (fpq_gemm_fp6_kernel.h)
        const int sb = piece / 3, ci = (piece % 3) * 64 + lane;
        const int r = ci / 6, pc = ci - 6 * r;          // row inside the super-block, physical chunk
        int c = pc - fp6_rot(r);
        c = c < 0 ? c + 6 : c;                          // logical chunk this lane fetches
        const int t = t0 + sb * 32 + r;
        voff[i] = (uint32_t)((t < T ? t : T - 1) - t0) * (uint32_t)a_row_bytes + (uint32_t)(c * 16);
      }
    } else if constexpr (W4) {                          // the weight side, rows dealt over the wavefront's NT tiles: a 16-row block
      const int wb = piece - APC, q = lane >> 2, kb = (lane & 3) ^ glds_chunk_perm(q);
      const int o = o0 + (wb / NT) * (16 * NT) + NT * q + wb % NT;
      voff[i] = (uint32_t)((o < O ? o : O - 1) - o0) * (uint32_t)w_row_bytes + (uint32_t)(kb * 16);
    } else {                                            // ... a super-block
      const int wp = piece - APC, sb = wp / 3, ci = (wp % 3) * 64 + lane;
      const int r = ci / 6, pc = ci - 6 * r;
      int c = pc - fp6_rot(r);
      c = c < 0 ? c + 6 : c;
      const int ti = 2 * sb + (r >> 4);                 // 16-row tile of the weight side
      const int o = o0 + (ti / NT) * (16 * NT) + NT * (r & 15) + ti % NT;
      voff[i] = (uint32_t)((o < O ? o : O - 1) - o0) * (uint32_t)w_row_bytes + (uint32_t)(c * 16);
    }
  }
#endif
#define FPQ_G6_ISSUE(g, buf)                                                                                        \
  _Pragma("unroll") for (int i_ = 0; i_ < PIECES; ++i_) {                                                           \
    const int piece_ = wave + 4 * i_;                                                                               \
    if (piece_ < NPC)   /* wavefront-uniform */                                                                     \
      FPQ_GLDS_LOAD(voff[i_], piece_ < APC ? a_base_g + (g) * a_step : w_base_g + (g) * w_step,                     \
                    smem + (buf) * STAGE + piece_ * 1024);                                                          \
  }
  FPQ_G6_ISSUE(0, 0);
#if FPQ_G6_KM
  FPQ_GEMM_KM_SCALE_TILES(sa, sw);
#else
  load_scale_tiles<Tsw, BM, BN, NTHR>(sa, sw, lsa, lsw, t0, o0, T, O, G, tid);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), the builtin: the compiler's scoreboard forgets the scale loads (gemm_fp4_glds_kernel)
#endif
#if FPQ_G6_FC1
  // the dual quantizer's bucket table, behind the scale tiles; visible after the first barrier of the main loop
  uint16_t* lut = (uint16_t*)(lsw + Gp * BN);
  lut16_stage(lut, xe.tab, xe.a.shift);
#endif

  // (OUT == 2: the fp16 bias is NULL, the q / k norm's fp32 bias replaces it)
#if !FPQ_G6_FC1 && FPQ_G6_OUT == 2
  FPQ_GEMM_LANE_BIAS(true, xe.bias, xe.q_scale);
#else
  FPQ_GEMM_LANE_BIAS(false, (const float*)nullptr, (const float*)nullptr);
#endif

  v4f_t acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = v4f_t{0, 0, 0, 0};

  // a 6-bit fragment: three 8-byte pieces inside a 16-row half of a super-block (foff); a nibble fragment: row lane & 15, chunk
  // lane >> 4 of a 16-row block (nib_off).  With nibble weights foff[] addresses the activation fragment alone and carries the
  // wavefront's activation base (one add less per read); otherwise it addresses the weight fragment too and the base stays in a_off.
  const int fr = lane & 15, kblk = lane >> 4;
  int foff[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int b = kblk * 24 + 8 * t;
    int pc = (b >> 4) + fp6_rot(fr);
    pc = pc >= 6 ? pc - 6 : pc;
    foff[t] = (W4 ? wm * MT * A_TILE : 0) + fr * 96 + pc * 16 + (b & 15);
  }
#define FPQ_G6_NIB_OFF ((fr << 6) + (((kblk ^ glds_chunk_perm(fr)) & 3) << 4))
  const int a_off = (W4 ? 0 : wm * MT * A_TILE) + (A4 ? FPQ_G6_NIB_OFF : 0);
  const int b_off = ABYTES + wn * NT * W_TILE + (W4 ? FPQ_G6_NIB_OFF : 0);
#undef FPQ_G6_NIB_OFF
  const int sa_off = wm * MT * 16 + 4 * kblk, sw_off = wn * NT * 16 + NT * fr;   // outputs 4q .. 4q+3: tile n holds 4q + n
  // the fragment of the 16-row tile at p_ (= stage + the side's offset + the tile's): one ds_read_b128 of nibbles or three ds_read_b64
#define FPQ_G6_READ(dst_, nibbles_, p_)                                                                             \
  do {                                                                                                              \
    if constexpr (nibbles_) {                                                                                       \
      FPQ_GEMM_READ_NIB(dst_, p_);                                                                                  \
    } else {                                                                                                        \
      const u32x2 q0_ = FPQ_LDS_READ64((p_) + foff[0]), q1_ = FPQ_LDS_READ64((p_) + foff[1]),                       \
                  q2_ = FPQ_LDS_READ64((p_) + foff[2]);                                                             \
      dst_ = v8i_t{(int)q0_[0], (int)q0_[1], (int)q1_[0], (int)q1_[1], (int)q2_[0], (int)q2_[1], 0, 0};             \
    }                                                                                                               \
  } while (0)
#define FPQ_G6_READ_A(dst_, st_, tile_) FPQ_G6_READ(dst_, A4, (st_) + (tile_) + a_off)
#define FPQ_G6_READ_W(dst_, st_, tile_) FPQ_G6_READ(dst_, W4, (st_) + b_off + (tile_))

  for (int g = 0; g < G; ++g) {   // the two-stage schedule of gemm_fp4_glds_kernel
    FPQ_GLDS_WAIT();
    FPQ_SYNC();   // stage g has landed; stage g^1's readers are done
    if (g + 1 < G) { FPQ_G6_ISSUE(g + 1, (g + 1) & 1); }
    const uint8_t* st = smem + (g & 1) * STAGE;
    FPQ_GEMM_GROUP(g, st, FPQ_G6_READ_A, FPQ_G6_READ_W, A_TILE, W_TILE, FA, FW);
  }
#undef FPQ_G6_READ
#undef FPQ_G6_READ_A
#undef FPQ_G6_READ_W
#undef FPQ_G6_ISSUE
#undef FPQ_G6_TSA

  // the register epilogue: the fc1 tail (the maxima exchange goes into stage buffer G & 1, which the last K group does not read
  // and nothing was loaded into after the group before it was read: the last issue fills buffer (G - 1) & 1; no gate / residual
  // tail: epi is not read), the split output (no gate / residual tail either), or the one tensor with the gate / residual tail
#if FPQ_G6_FC1 == 2
  FPQ_GEMM_FC1_TAIL_X(STAGE, true);   // the dual pair without a global clamp: a NaN stays out of the maxima
#elif FPQ_G6_FC1
  FPQ_GEMM_FC1_TAIL(STAGE);
#elif FPQ_G6_OUT == 3
  FPQ_GEMM_SQERR_EPILOGUE(smem + (G & 1) * STAGE);   // (scratch: the idle stage buffer, as the fc1 tail's)
#elif FPQ_G6_OUT
  FPQ_GEMM_REG_EPILOGUE(FPQ_G6_OUT == 2, false, true);   // (q / k norm, gate / residual tail, split output)
#else
  FPQ_GEMM_REG_EPILOGUE(false, true, false);
#endif
}
#undef FPQ_G6_KERNEL
#undef FPQ_G6_FC1
#undef FPQ_G6_OUT
#undef FPQ_G6_KM
#undef FPQ_G6_W4
