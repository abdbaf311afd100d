// Textually included into gemm_pair_8ph_kernel (all 2 x 4 blocks of a wave's 64 x 128) and gemm_pair_8ph_fixup_kernel (one 32 x 32 block).
// Expects in scope: p, acc[EP_NI][EP_NJ], em0, en0, wr, wc, fr, fh, acc_scale, out_amax, ACT, RES and the constants EP_NI / EP_NJ (row / column
// blocks in acc), EP_FULL (whether a wave with all its 64 rows inside M takes the unmasked form); EP_I0 / EP_J0 = the block acc[0][0] is
// (ints, need not be constant).
// Epilogue straight from the accumulators: lane (fr, fh) holds column 32 j + fr of the wave's 128 (blocks j = 0..3), rows
// 32 i + (r & 3) + 8 (r >> 2) + 4 fh: one register = two 128-B row segments per wave instruction.  Rows >= M fall off
// the descriptors' extents; residual in units of (row block, column-block pair), the next unit's in flight behind
// the current one.
{
    constexpr int EP_JG = EP_NJ >= 2 ? 2 : 1, EP_UPR = EP_NJ / EP_JG, EP_NU = EP_NI * EP_UPR;   // column blocks per unit, units per row block, units
    const int mw = em0 + wr * 64;
    const long long rows_left = (long long)p.M - mw;
    const __amdgpu_buffer_rsrc_t rsC = desc(p.c, rows_left > 0 ? ((rows_left - 1) * p.ldc + p.N) * 4 + (long long)mw * p.ldc * 4 : 0,
                                            (long long)mw * p.ldc * 4);
    const __amdgpu_buffer_rsrc_t rsR = RES ? desc(p.res, rows_left > 0 ? ((rows_left - 1) * p.ldr + p.N) * 4 + (long long)mw * p.ldr * 4 : 0,
                                                  (long long)mw * p.ldr * 4)
                                           : __builtin_amdgcn_make_buffer_rsrc((void*)p.c, 0, 0, 0x00020000);
    unsigned vc[EP_NJ], vr[EP_NJ];
    float sv[EP_NJ], bv[EP_NJ];
#pragma unroll
    for (int j = 0; j < EP_NJ; ++j) {
        const int n = en0 + wc * 128 + 32 * (EP_J0 + j) + fr;
        vc[j] = (unsigned)((4 * fh * p.ldc + n) * 4); vr[j] = (unsigned)((4 * fh * p.ldr + n) * 4);
        sv[j] = (p.oscale ? p.oscale[n] : 1.f) * acc_scale;
        bv[j] = p.bias ? p.bias[n] : 0.f;
    }
    float rv[RES ? 2 : 1][EP_JG][16];
    // Rows >= M of a ragged last tile are masked BY LANE (an out-of-range voffset), not left to the descriptor's extent:
    // their row offset travels in soffset, which can exceed num_records there, and the range check is
    // `offset >= num_records - soffset`.  A full tile (FULL) pays nothing for it.
    const int row_lim = (int)(rows_left < 1024 ? rows_left : 1024) - 4 * fh;     // row u of this lane is valid iff u < row_lim
    auto epilogue = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        auto load_res = [&](int u, int slot) {                    // unit u = (i = u / EP_UPR, column blocks EP_JG (u % EP_UPR) ..)
#pragma unroll
            for (int jj = 0; jj < EP_JG; ++jj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ru = 32 * (EP_I0 + u / EP_UPR) + (r & 3) + 8 * (r >> 2);
                    const unsigned vo = (FULL || ru < row_lim) ? vr[EP_JG * (u % EP_UPR) + jj] : OOR;
                    rv[slot][jj][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsR, vo, (unsigned)(ru * p.ldr * 4), 0));
                }
        };
        if constexpr (RES) load_res(0, 0);
#pragma unroll
        for (int u = 0; u < EP_NU; ++u) {
            if constexpr (RES) { if (u + 1 < EP_NU) load_res(u + 1, (u + 1) & 1); }
            const int i = u / EP_UPR;
#pragma unroll
            for (int jj = 0; jj < EP_JG; ++jj) {
                const int j = EP_JG * (u % EP_UPR) + jj;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = (acc[i][j][r] * sv[j] + bv[j]) * p.alpha;
                    if constexpr (RES) v += rv[u & 1][jj][r];
                    if (ACT == DBMM_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (ACT == DBMM_ACT_QUICKGELU) v = v / (1.f + expf(-1.702f * v));
                    const int ru = 32 * (EP_I0 + i) + (r & 3) + 8 * (r >> 2);
                    const bool valid = FULL || ru < row_lim;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC, valid ? vc[j] : OOR,
                                                          (unsigned)(ru * p.ldc * 4), 0);
                    if (valid) out_amax = fmaxf(out_amax, fabsf(v));
                }
            }
        }
    };
    if (EP_FULL && rows_left >= 64) epilogue(std::true_type{}); else epilogue(std::false_type{});
}
