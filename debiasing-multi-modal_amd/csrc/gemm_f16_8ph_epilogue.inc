// Textually included into gemm_f16_8ph_kernel (all four 32-row blocks of a wave's 128 x 64) and gemm_f16_8ph_fixup_kernel (one block).
// Expects in scope: p, acc[EP_NI][2], em0, en0, wr, wc, fr, fh, ACT, RES and the constants EP_NI (row blocks in acc), EP_FULL (whether a wave
// with all its 128 rows inside M takes the unmasked form); EP_I0 = the 32-row block acc[0] is (an int, need not be constant).
// Epilogue straight from the accumulators, no LDS: lane (fr, fh) holds output columns 2 fr and 2 fr + 1 (blocks j = 0 / 1,
// see ring_rows) of rows 32 i + (r & 3) + 8 (r >> 2) + 4 fh: one packed dword per register, 32 lanes = one
// whole 128-B row segment, two rows per wave instruction -- the full-rate access shape, residual loads likewise.
// (Through the LDS transpose of gemm_f16_kernel the 68 KB of fp32 staging writes cost as much as the MFMAs of two K
//  tiles; with swapped MFMA operands -- a lane owning 4 columns of ITS row, 8-B accesses to 32 different lines per
//  instruction -- the vector-memory path made it slower still: 848 -> 663 TF on the out-projection shape.)
{
    const int n = en0 + wc * 64 + 2 * fr;
    float bn0 = 0.f, bn1 = 0.f, sn0 = 1.f, sn1 = 1.f;
    if (p.bias) { bn0 = p.bias[n]; bn1 = p.bias[n + 1]; }
    if (p.oscale) { sn0 = p.oscale[n]; sn1 = p.oscale[n + 1]; }
    const bool rf = p.res_first != 0;
    // descriptors rebased to the wave's first row: the extent ends with the last valid row, so rows past M are dropped
    // by the hardware (no branches); lane offset = its column pair + its half's 4-row step, the row of a register is a
    // wave-uniform scalar offset
    const int mw = em0 + wr * 128;
    const long long rows_left = (long long)p.M - mw;
    const __amdgpu_buffer_rsrc_t rsC = desc(p.c, rows_left > 0 ? ((rows_left - 1) * p.ldc + p.N) * 2 + (long long)mw * p.ldc * 2 : 0, (long long)mw * p.ldc * 2);
    const __amdgpu_buffer_rsrc_t rsR = p.res ? desc(p.res, rows_left > 0 ? ((rows_left - 1) * p.ldr + p.N) * 2 + (long long)mw * p.ldr * 2 : 0, (long long)mw * p.ldr * 2)
                                             : __builtin_amdgcn_make_buffer_rsrc((void*)p.c, 0, 0, 0x00020000);
    const unsigned vc = (unsigned)((4 * fh * p.ldc + n) * 2), vr = (unsigned)((4 * fh * p.ldr + n) * 2);
    // Rows >= M of a ragged last tile are masked BY LANE (an out-of-range voffset) instead of being left to the extent:
    // their row offset travels in soffset, which can exceed num_records there (range check: offset >= num_records -
    // soffset).  A full tile pays nothing.
    const int row_lim = (int)(rows_left < 1024 ? rows_left : 1024) - 4 * fh;     // row u of this lane is valid iff u < row_lim
    auto epilogue = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        // all residual loads in flight together (the fragment registers are dead here): one round trip, not four
        unsigned rvv[RES ? EP_NI : 1][16];
        if constexpr (RES) {
#pragma unroll
            for (int i = 0; i < EP_NI; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ru = 32 * (EP_I0 + i) + (r & 3) + 8 * (r >> 2);
                    rvv[i][r] = __builtin_amdgcn_raw_buffer_load_b32(rsR, (FULL || ru < row_lim) ? vr : OOR, (unsigned)(ru * p.ldr * 2), 0);
                }
        }
#pragma unroll
        for (int i = 0; i < EP_NI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f16x2 rh = __builtin_bit_cast(f16x2, RES ? rvv[i][r] : 0u);
                const float r0 = RES ? (float)rh[0] : 0.f, r1 = RES ? (float)rh[1] : 0.f;
                float o0 = act_f(fmaf(acc[i][0][r], sn0, bn0) + (rf ? r0 : 0.f), ACT), o1 = act_f(fmaf(acc[i][1][r], sn1, bn1) + (rf ? r1 : 0.f), ACT);
                if (RES) { o0 += rf ? 0.f : r0; o1 += rf ? 0.f : r1; }
                if (GF16_ABL & 2) { asm volatile("" ::"v"(acc[i][0][r]), "v"(acc[i][1][r]), "v"(rh)); continue; }
                if (GF16_ABL & 1) { asm volatile("" ::"v"(pack2(o0, o1))); continue; }
                const int ru = 32 * (EP_I0 + i) + (r & 3) + 8 * (r >> 2);
                __builtin_amdgcn_raw_buffer_store_b32(pack2(o0, o1), rsC, (FULL || ru < row_lim) ? vc : OOR, (unsigned)(ru * p.ldc * 2), 0);
            }
        }
    };
    if (EP_FULL && rows_left >= 128) epilogue(std::true_type{}); else epilogue(std::false_type{});
}
