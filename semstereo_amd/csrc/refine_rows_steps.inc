// Steps 2 and 3 of the row kernels (disparity_refine.hip, disparity_fill2d.hip), as program text: included INSIDE the kernel's row loop,
// between the barrier after the row's bytes are in LDS and the barrier before step 4.  A function was tried first: inlined, it changed
// the row kernel's register allocation and made the axes="rows" call 1 % slower at 1 x 4096^2 (profiles/EXPERIMENTS.md part AI); as
// text the row kernel's object code is what it was.  In scope at the point of inclusion:
//   flag     the bytes of a row of Wp = chunk * BLOCK columns in LDS (u8*; bits 0-3 the class, NCLS for none; SRC the source bit)
//   cand     2 * QR 16-byte words in LDS (uint4*), QR = Wp / 4
//   scratch  SCRATCH ints in LDS (int*)
//   chunk    the columns of a thread, a multiple of 4; c0 = threadIdx.x * chunk, the thread's first column
// Afterwards cand[q] holds the left candidates of columns 4 q .. 4 q + 3 (own class x 4, any class x 4, as 16-bit columns, NOCOL for
// none) and cand[QR + q] the right ones.  No include guard: the text is meant to appear once per kernel.
        // 2 ---- the left candidates: the last source column per class (0 .. 7) and of any class (8), -1 for none
        int last[NCLS + 1];
#pragma unroll
        for (int k = 0; k <= NCLS; ++k) last[k] = -1;
        for (int g = 0; g < chunk; g += 4) {
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flag + c0 + g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = (int)((f4 >> (8 * j)) & 255u), x = c0 + g + j;
                if (f & SRC) {
                    last[NCLS] = x;
#pragma unroll
                    for (int k = 0; k < NCLS; ++k) last[k] = (f & 15) == k ? x : last[k];
                }
            }
        }
        block_scan_exclusive<NCLS + 1, false>(last, -1, scratch);
        for (int g = 0; g < chunk; g += 4) {
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flag + c0 + g);
            unsigned own[4], any[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = (int)((f4 >> (8 * j)) & 255u), x = c0 + g + j;
                int mine = -1;
#pragma unroll
                for (int k = 0; k < NCLS; ++k) mine = (f & 15) == k ? last[k] : mine;
                own[j] = (unsigned)mine & 0xFFFFu, any[j] = (unsigned)last[NCLS] & 0xFFFFu;          // (-1 becomes NOCOL)
                if (f & SRC) {
                    last[NCLS] = x;
#pragma unroll
                    for (int k = 0; k < NCLS; ++k) last[k] = (f & 15) == k ? x : last[k];
                }
            }
            cand[(c0 + g) >> 2] = make_uint4(own[0] | own[1] << 16, own[2] | own[3] << 16, any[0] | any[1] << 16, any[2] | any[3] << 16);
        }
        // 3 ---- the right candidates: the first source column per class and of any class, NOCOL for none
        int first[NCLS + 1];
#pragma unroll
        for (int k = 0; k <= NCLS; ++k) first[k] = NOCOL;
        for (int g = chunk - 4; g >= 0; g -= 4) {
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flag + c0 + g);
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const int f = (int)((f4 >> (8 * j)) & 255u), x = c0 + g + j;
                if (f & SRC) {
                    first[NCLS] = x;
#pragma unroll
                    for (int k = 0; k < NCLS; ++k) first[k] = (f & 15) == k ? x : first[k];
                }
            }
        }
        block_scan_exclusive<NCLS + 1, true>(first, NOCOL, scratch);
        for (int g = chunk - 4; g >= 0; g -= 4) {
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flag + c0 + g);
            unsigned own[4], any[4];
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const int f = (int)((f4 >> (8 * j)) & 255u), x = c0 + g + j;
                int mine = NOCOL;
#pragma unroll
                for (int k = 0; k < NCLS; ++k) mine = (f & 15) == k ? first[k] : mine;
                own[j] = (unsigned)mine, any[j] = (unsigned)first[NCLS];
                if (f & SRC) {
                    first[NCLS] = x;
#pragma unroll
                    for (int k = 0; k < NCLS; ++k) first[k] = (f & 15) == k ? x : first[k];
                }
            }
            cand[QR + ((c0 + g) >> 2)] = make_uint4(own[0] | own[1] << 16, own[2] | own[3] << 16, any[0] | any[1] << 16, any[2] | any[3] << 16);
        }
