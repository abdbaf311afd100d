// Textually included into conv3x3_halo8_kernel, conv3x3_halo8n_kernel (all blocks of a wave) and conv3x3_halo8_fixup_kernel (one 32 x 32 block)
// (as a function taking the accumulators by reference hipcc spilled ~260 registers around the call).
// Expects in scope: p, acc[EP_NI][EP_NB], em0, en0, wr, wc, fr, fh, acc_scale, out_amax, POOL, ACT and the constants EP_NI / EP_NB (row blocks /
// 32-column blocks in acc: 2 x 4 | 2 x 2 | 1 x 1), EP_WCOLS (columns per wave: 128 | 64); EP_I0 / EP_J0 = the block acc[0][0] is (ints, need not
// be constant).
// Epilogue straight from the accumulators: lane (fr, fh) holds column 32 j + fr of the wave's 128 (blocks j = 0..3), rows
// 32 i + (r & 3) + 8 (r >> 2) + 4 fh.  Plain: one register = two 128-B row segments per wave instruction.  POOL: registers
// 4 k .. 4 k + 3 are the four pixels (dy, dx) of window 8 i + 2 k + fh -- ReLU each, sum in (dy, dx) order, * 0.25 (the
// arithmetic of igemm_epilogue.inc's pooled path), one pooled row segment per lane half.
{
    float sv[EP_NB], bv[EP_NB];
#pragma unroll
    for (int j = 0; j < EP_NB; ++j) {
        const int n = en0 + wc * EP_WCOLS + 32 * (EP_J0 + j) + fr;
        sv[j] = (p.oscale ? p.oscale[n] : 1.f) * acc_scale;
        bv[j] = p.bias ? p.bias[n] : 0.f;
    }
    if constexpr (POOL) {
        const int mpw = (em0 + wr * 64) >> 2;                         // first pooled row of this wave (16 of them)
        const long long rows_left = (long long)(p.M >> 2) - mpw;
        const __amdgpu_buffer_rsrc_t rsC = desc(p.c, rows_left > 0 ? ((rows_left - 1) * p.ldc + p.N) * 4 + (long long)mpw * p.ldc * 4 : 0,
                                                (long long)mpw * p.ldc * 4);
        const int row_lim = (int)(rows_left < 1024 ? rows_left : 1024) - fh;          // pooled row u of this lane is valid iff u < row_lim
#pragma unroll
        for (int i = 0; i < EP_NI; ++i)
#pragma unroll
            for (int j = 0; j < EP_NB; ++j) {
                const unsigned vc = (unsigned)((fh * p.ldc + en0 + wc * EP_WCOLS + 32 * (EP_J0 + j) + fr) * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float sum = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float v = acc[i][j][4 * k + q] * sv[j] + bv[j];
                        if (ACT == DBMM_ACT_RELU) v = fmaxf(v, 0.f);
                        sum += v;
                    }
                    sum *= 0.25f;
                    const int u = 8 * (EP_I0 + i) + 2 * k;
                    const bool valid = u < row_lim;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sum), rsC, valid ? vc : OOR, (unsigned)(u * p.ldc * 4), 0);
                    if (valid) out_amax = fmaxf(out_amax, fabsf(sum));
                }
            }
    } else {
        const int mw = em0 + wr * 64;
        const long long rows_left = (long long)p.M - mw;
        const __amdgpu_buffer_rsrc_t rsC = desc(p.c, rows_left > 0 ? ((rows_left - 1) * p.ldc + p.N) * 4 + (long long)mw * p.ldc * 4 : 0,
                                                (long long)mw * p.ldc * 4);
        const int row_lim = (int)(rows_left < 1024 ? rows_left : 1024) - 4 * fh;      // row u of this lane is valid iff u < row_lim
#pragma unroll
        for (int i = 0; i < EP_NI; ++i)
#pragma unroll
            for (int j = 0; j < EP_NB; ++j) {
                const unsigned vc = (unsigned)((4 * fh * p.ldc + en0 + wc * EP_WCOLS + 32 * (EP_J0 + j) + fr) * 4);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j][r] * sv[j] + bv[j];
                    if (ACT == DBMM_ACT_RELU) v = fmaxf(v, 0.f);
                    const int u = 32 * (EP_I0 + i) + (r & 3) + 8 * (r >> 2);
                    const bool valid = u < row_lim;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC, valid ? vc : OOR, (unsigned)(u * p.ldc * 4), 0);
                    if (valid) out_amax = fmaxf(out_amax, fabsf(v));
                }
            }
    }
}
