// Every conv_x3_f16 and conv_x3_wr instance the library builds, written once (an X-macro list).
// conv_x3.hip expands it into the table from a choice (x3_select.h) to its launcher, and so
// instantiates exactly these kernels; x3_select.cpp expands it into the forms of each instance.
//
//   X3_F16(KS, WAVES_M, WAVES_N, WM, WN, VAR, OCC, FORMS)   conv_x3_f16, VAR without its form bits
//   X3_WR(KS, WN, DEPTH, FORMS)                             conv_x3_wr
// FORMS: 1 three-term (fp32-accurate), 2 one-term (ISL_PREC_FP16), 4 one-term on fp16 buffers
// (ISL_ACT_FP16).  No fp16-storage form: K ranges across blocks (VAR 2048), the fold (8192), the
// stamps (16384), the 96-pixel 7x7 tiles and the wave-range kernel; the 16x16x32 row union
// (131072) is three-term only.
// The development instances (ISLPOSE_DEV: tools/convbench, tools/libislpose_dev.so) are the
// stamps 16384, M16 131072, the fold 8192, small-grid 4096 and the ranged half-channel blocks.
//
// The includer defines X3_F16 and X3_WR; the helper macros below are undefined again at the end.

#define X3_K13(M, ...) M(1, __VA_ARGS__) M(3, __VA_ARGS__)
#define X3_K137(M, ...) M(1, __VA_ARGS__) M(3, __VA_ARGS__) M(7, __VA_ARGS__)
// a loop of the 128-pixel family with its K ranges across blocks, in one block, or none
#define X3_TRIPLE(KS, A, B, C, D, BASE, OCC, FORMS)          \
  X3_F16(KS, A, B, C, D, 2048 | (BASE), OCC, (FORMS) & 3)    \
  X3_F16(KS, A, B, C, D, 1024 | (BASE), OCC, FORMS)          \
  X3_F16(KS, A, B, C, D, BASE, OCC, FORMS)

// --- 3x3 on the row union (512-pixel tiles) ---
#ifdef ISLPOSE_DEV
X3_F16(3, 2, 8, 2, 2, 512 | 16384, 4, 3)
X3_F16(3, 1, 16, 3, 1, 512 | 16384, 4, 3)
X3_F16(3, 2, 8, 2, 2, 512 | 32768 | 131072, 4, 1)
X3_F16(3, 2, 8, 2, 2, 512 | 131072, 4, 1)
#endif
X3_F16(3, 2, 8, 2, 2, 512 | 32768, 4, 7)
X3_F16(3, 2, 8, 2, 2, 512, 4, 7)
X3_F16(3, 1, 16, 3, 1, 512, 4, 7)
X3_F16(3, 2, 8, 1, 2, 512, 4, 7)
X3_F16(3, 1, 16, 1, 1, 512, 4, 7)
// --- 1x1 on 256-channel tiles, two chunk pairs per step ---
X3_F16(1, 4, 4, 2, 2, 4096, 1, 7)
// --- 1x1 / 3x3 on the generic 512- / 256-pixel tiles ---
X3_F16(3, 2, 8, 2, 2, 32768, 4, 7)
X3_F16(3, 1, 8, 2, 1, 32768, 2, 7)
X3_K13(X3_F16, 1, 8, 2, 1, 0, 2, 7)     // 8 waves of 64co x 32px, 256 px
X3_K13(X3_F16, 2, 8, 2, 2, 0, 4, 7)     // 16 waves, 64co x 64px each
X3_K13(X3_F16, 1, 16, 3, 1, 0, 4, 7)    // 16 waves, 96co x 32px
X3_K13(X3_F16, 2, 8, 1, 2, 0, 4, 7)     // 16 waves, 32co x 64px
X3_K13(X3_F16, 1, 16, 1, 1, 0, 4, 7)    // 16 waves, 32co x 32px
// --- 7x7, 128-channel tiles without K ranges ---
X3_F16(7, 2, 3, 1, 1, 256 | 128, 1, 3)
X3_F16(7, 2, 2, 1, 1, 256 | 128, 1, 7)
X3_F16(7, 2, 2, 1, 1, 256, 4, 7)
X3_F16(7, 2, 6, 2, 2, 65536, 1, 7)      // 12 waves, 384 px
X3_F16(7, 2, 4, 2, 2, 0, 1, 7)
X3_F16(7, 2, 4, 2, 1, 0, 1, 7)
// --- the 128-pixel family: 8 / 12 waves on 128- / 96-channel tiles ---
#ifdef ISLPOSE_DEV
X3_K13(X3_TRIPLE, 2, 4, 2, 1, 8192, 2, 3)
X3_K13(X3_TRIPLE, 3, 4, 1, 1, 8192, 2, 3)
#endif
X3_K13(X3_F16, 2, 4, 2, 1, 1024 | 32, 1, 7)   // two K groups of 8 waves
X3_K137(X3_F16, 1, 4, 2, 1, 256, 4, 7)        // half-channel blocks
X3_K13(X3_TRIPLE, 2, 4, 2, 1, 128, 1, 7)      // two K steps ahead
X3_K13(X3_TRIPLE, 3, 4, 1, 1, 128, 1, 7)
#ifdef ISLPOSE_DEV
X3_K13(X3_TRIPLE, 2, 4, 2, 1, 4096, 2, 7)
X3_K13(X3_TRIPLE, 3, 4, 1, 1, 4096, 2, 7)
#endif
X3_F16(7, 2, 2, 1, 1, 2048 | 256 | 128, 1, 3)
X3_K137(X3_F16, 2, 2, 1, 1, 2048 | 256, 4, 3)
X3_K137(X3_F16, 1, 4, 2, 1, 2048 | 256, 4, 3)
#ifdef ISLPOSE_DEV
X3_K137(X3_F16, 1, 4, 2, 1, 1024 | 256, 4, 7)
#endif
X3_K137(X3_TRIPLE, 2, 4, 2, 1, 0, 2, 7)       // 8 waves of 64co x 32px
X3_K137(X3_F16, 3, 2, 1, 1, 2048, 4, 3)       // 6 waves on 64-pixel tiles
X3_K137(X3_TRIPLE, 3, 4, 1, 1, 0, 2, 7)       // 12 waves of 32co x 32px
// --- the 128-pixel family: 4 waves (ISLPOSE_X3_S8=0, and the 64- / 32-channel tiles) ---
X3_K137(X3_TRIPLE, 2, 2, 2, 2, 0, 2, 7)
X3_K137(X3_TRIPLE, 1, 4, 3, 1, 0, 2, 7)
X3_K137(X3_TRIPLE, 1, 4, 2, 1, 0, 2, 7)
X3_K137(X3_TRIPLE, 1, 4, 1, 1, 0, 2, 7)
// --- the fused 1x1 pair: one tile of every Mconv6 channel (512, 256, 128) ---
X3_F16(1, 8, 2, 2, 2, 16, 4, 7)
X3_F16(1, 4, 4, 2, 2, 16, 4, 7)
X3_F16(1, 2, 8, 2, 2, 16, 4, 7)
// --- the wave-range kernel: 32- and 64-pixel tiles ---
X3_K137(X3_WR, 1, 12, 3)
X3_K137(X3_WR, 2, 8, 3)

#undef X3_K13
#undef X3_K137
#undef X3_TRIPLE
